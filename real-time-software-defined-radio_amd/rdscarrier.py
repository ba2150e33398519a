"""RDS carrier phase recovery on the host, pure Python / numpy (no GPU, no libsdr).

RdsCarrierPhase is the specification of the device stage (RdsCarrierBank, csrc/rds_carrier.hip):
one stream's RRC rows i and q (float32, 24 samples a symbol) -> one float32 row, the samples
projected onto the axis the data lie on -- what RdsSymbolClock.process and RdsClockBank.process_dev
take.  The clock, the link layer and the block synchroniser read the in-phase row only; with the
57 kHz carrier's phase off (another station, other filters, another PLL phase adjustment) the symbol
energy moves into q, and at 90 degrees i holds noise.  This stage finds the axis from both rows and
turns it onto i.  n samples in give n samples out.

Every decision is made from exact quantities and every rounded operation is one IEEE operation, so
the device equals it bit for bit, whether or not the compiler fuses a * b + c.

Segments.  The stream's samples are cut into segments of SEG = 768 samples (32 symbols) on the
absolute sample grid: the clock's segments.

Moments of a complete segment g.  The float32 samples widened to f64, a pair with a non-finite value
on either side counting as (0, 0): Sii_g, Sqq_g, Siq_g from the products i i, q q, i q -- for each
offset p = 0 .. 23 the sum over j = 0 .. 31, ascending, of the product at sample 768 g + 24 j + p,
then those 24 values summed with p ascending.  (A product of two float32 values is exact in f64.)

Window.  For g >= 1, w = min(window, g); A, B, C = the sums of Sii, Sqq, Siq over segments
g - w .. g - 1, oldest first; P = A - B, Q = 2 C.

Direction.  khat in 0 .. 31 is the sector of the doubled angle atan2(Q, P), sectors 11.25 degrees
wide and centred on the multiples of 11.25 degrees, found without a transcendental: a = |P|,
b = |Q|, swapped if b > a; if not a > 0 there is no direction: the segment holds kappa and `holds`
counts it.  m = how many of the four thresholds t = tan(pi/32), tan(3 pi/32), tan(5 pi/32),
tan(7 pi/32) (THRESHOLDS: decimal literals) satisfy b > a t; m = 8 - m if swapped; m = 16 - m if
P < 0; m = (32 - m) mod 32 if Q < 0.

Tracking.  The axis index kappa in 0 .. 63 runs over the full circle, angle pi kappa / 32.  Segment
0 uses kappa = 0; segment 1 sets kappa = khat; later d = ((khat - kappa + 16) mod 32) - 16 and kappa
moves one step up (mod 64) if d >= 2, one down if d <= -2, else stays: a dead band of one sector.
The target is known mod 32 only (the data axis has no sign); kappa moves the shorter way and never
jumps, so the output never changes sign under the differential decoder.  The slew is at most one
sector a segment: 5.625 degrees per 13.5 ms, about 417 degrees/s -- a carrier turning at 300
degrees/s is followed, one at 500 degrees/s is lost.

Axis table.  AXES: 64 float32 pairs (c, s).  Entries 0 .. 8 are cos and sin of pi kappa / 32 in f64
rounded to float32, entry 0 exactly (1, 0) and entry 8 float32(sqrt(1/2)) twice; the other 55 follow
by symmetry (swap, negate), so 90 degrees is exactly (0, 1) and kappa = 0 the identity.

Output.  For every sample v of segment g, complete or not,
y[v] = float32(f64(c) f64(i[v]) + f64(s) f64(q[v])) with (c, s) = AXES[kappa_g], the samples as they
are, non-finite ones included.  Both products are exact in f64, so the sum is rounded once.  With
kappa = 0, y equals i wherever q is finite.  The axis of an incomplete segment depends on complete
segments only, so it is the same whenever the segment's samples arrive: any split of a stream into
calls gives the same output.
"""
from __future__ import annotations

import numpy as np

SPS = 24
SEG_SYMBOLS = 32
SEG = SPS * SEG_SYMBOLS  # 768
MAX_WINDOW = 16
SECTORS = 32             # directions of the doubled angle; 2 SECTORS axis indices

# tan(pi/32), tan(3 pi/32), tan(5 pi/32), tan(7 pi/32): the literals of csrc/rds_carrier.hip
THRESHOLDS = (0.098491403357164248, 0.3033466836073424, 0.53451113595079158, 0.82067879082866024)


def _axes() -> np.ndarray:
    first = np.empty((9, 2), dtype=np.float32)
    for k in range(9):
        first[k] = (np.float32(np.cos(np.pi * k / 32)), np.float32(np.sin(np.pi * k / 32)))
    first[0] = (1.0, 0.0)
    first[8] = np.float32(np.sqrt(0.5))
    out = np.empty((64, 2), dtype=np.float32)
    for k in range(64):
        r, quarter = k % 16, k // 16
        c, s = first[r] if r <= 8 else first[16 - r][::-1]
        for _ in range(quarter):                                   # a quarter turn: (c, s) -> (-s, c)
            c, s = -s, c
        out[k] = (c, s)
    out += np.float32(0.0)                                         # no negative zeros
    out.setflags(write=False)
    return out


AXES = _axes()


def sector(P: float, Q: float):
    """khat in 0 .. 31, the sector of atan2(Q, P), or None where there is no direction"""
    P, Q = float(P), float(Q)
    a, b = abs(P), abs(Q)
    swapped = b > a
    if swapped:
        a, b = b, a
    if not a > 0:
        return None
    m = sum(1 for t in THRESHOLDS if b > a * t)
    if swapped:
        m = 8 - m
    if P < 0:
        m = 16 - m
    if Q < 0:
        m = (32 - m) % 32
    return m


def step_kappa(kappa: int, khat: int) -> int:
    """kappa moved one step towards khat (known mod 32) the shorter way, or left inside the dead band"""
    d = ((khat - kappa + 16) % 32) - 16
    if d >= 2:
        return (kappa + 1) % 64
    if d <= -2:
        return (kappa - 1) % 64
    return kappa


class RdsCarrierPhase:
    """Carrier phase recovery of one stream.  process(i, q) takes any number of float32 sample
    pairs (0 included) and returns as many float32 samples; any split of a stream into calls gives
    the same output.  `kappas` is the axis index of every segment the last call wrote samples of.

    window: 1 .. 16 segments of moments behind the direction (default 8).  The axis follows a
    carrier that turns at up to about 417 degrees/s (one sector of 5.625 degrees a segment): 300
    degrees/s is tracked, 500 degrees/s is lost."""

    def __init__(self, window: int = 8):
        if not 1 <= int(window) <= MAX_WINDOW:
            raise ValueError(f"window={window} outside [1, {MAX_WINDOW}]")
        self.window = int(window)
        self.reset()

    def reset(self):
        self._ti = np.zeros(0, dtype=np.float32)       # the samples of the incomplete segment
        self._tq = np.zeros(0, dtype=np.float32)
        self._M = []                                   # the last MAX_WINDOW moment triples
        self._last = (0.0, 0.0, 0.0)
        self.consumed = self.segments = 0
        self.kappa = 0
        self.steps_forward = self.steps_back = self.holds = self.wraps = 0
        self.kappas = []

    def state(self) -> tuple:
        """(consumed samples, complete segments, kappa of the last complete segment, steps forward,
        steps back, holds, wraps 63 <-> 0)"""
        return (self.consumed, self.segments, self.kappa, self.steps_forward, self.steps_back, self.holds, self.wraps)

    def moments(self) -> tuple:
        """(A, B, C) of the window behind the last complete segment's direction (zeros before
        segment 1): sqrt((A - B)^2 + (2 C)^2) / (A + B) is a lock measure"""
        return self._last

    def _next(self, count: bool) -> int:
        """the axis index of segment number self.segments"""
        g, kappa = self.segments, self.kappa
        if g == 0:
            return 0
        A = B = C = 0.0
        for sii, sqq, siq in self._M[-min(self.window, g):]:
            A += sii
            B += sqq
            C += siq
        khat = sector(A - B, 2.0 * C)
        if khat is None:
            new = kappa
        elif g == 1:
            new = khat
        else:
            new = step_kappa(kappa, khat)
        if count:
            self._last = (A, B, C)
            self.holds += khat is None
            if g > 1 and new != kappa:
                up = new == (kappa + 1) % 64
                self.steps_forward += up
                self.steps_back += not up
                self.wraps += (up and new == 0) or (not up and new == 63)
        return new

    @staticmethod
    def _sums(v, G):
        v = v.reshape(G, SEG_SYMBOLS, SPS)
        e = np.zeros((G, SPS))
        for j in range(SEG_SYMBOLS):
            e += v[:, j, :]
        t = np.zeros(G)
        for p in range(SPS):
            t += e[:, p]
        return t

    def process(self, i, q) -> np.ndarray:
        i = np.ascontiguousarray(i, dtype=np.float32).ravel()
        q = np.ascontiguousarray(q, dtype=np.float32).ravel()
        if len(i) != len(q):
            raise ValueError(f"{len(i)} samples of i, {len(q)} of q")
        n, t = len(i), len(self._ti)
        ri, rq = np.concatenate([self._ti, i]), np.concatenate([self._tq, q])
        G = len(ri) // SEG
        if G:
            fi, fq = ri[:G * SEG].astype(np.float64), rq[:G * SEG].astype(np.float64)
            bad = ~(np.isfinite(fi) & np.isfinite(fq))
            fi[bad] = 0.0
            fq[bad] = 0.0
            M = np.stack([self._sums(fi * fi, G), self._sums(fq * fq, G), self._sums(fi * fq, G)], axis=1)
        y = np.empty(n, dtype=np.float32)
        self.kappas = []
        for g in range(G + 1):
            lo, hi = max(g * SEG - t, 0), min((g + 1) * SEG - t, n)
            kappa = self._next(count=g < G)
            if hi > lo:
                c, s = (np.float64(v) for v in AXES[kappa])
                with np.errstate(invalid="ignore", over="ignore"):
                    y[lo:hi] = (c * i[lo:hi].astype(np.float64) + s * q[lo:hi].astype(np.float64)).astype(np.float32)
                self.kappas.append(kappa)
            if g < G:
                self.kappa = kappa
                self._M = (self._M + [tuple(float(v) for v in M[g])])[-MAX_WINDOW:]
                self.segments += 1
        self.consumed += n
        self._ti, self._tq = ri[G * SEG:].copy(), rq[G * SEG:].copy()
        return y
