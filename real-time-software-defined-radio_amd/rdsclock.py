"""RDS symbol clock recovery on the host, pure Python / numpy (no GPU, no libsdr).

RdsSymbolClock is the specification of the device stage (RdsClockBank, csrc/rds_clock.hip): one
stream's in-phase RRC samples (float32, 24 a symbol) -> differential bits, byte per bit -- what
RdsBlockSync.process and RdsSyncBank.process_dev take.  Where the link layer (RdsLinkLayer,
RdsLinkBank) fixes the sampling offset on the first 24 samples for ever, this stage follows the
symbol clock, so a receiver whose crystal is off keeps its bits.

Every decision is made from exact quantities -- squares of float32 samples summed in float64 in a
stated order, integer counts, comparisons of float32 samples -- so the device equals it bit for bit.

The stream's samples x[0], x[1], ... are cut into segments of SEG = 768 samples (32 symbols) on the
absolute sample grid; only complete segments are worked on, the rest waits for the next call.

Energy.  E_g[p] = sum over j = 0 .. 31, ascending, of x[768 g + 24 j + p]^2 in float64, a
non-finite sample counting as 0.  A_g[p] = E_(g-w+1)[p] + ... + E_g[p] over the last
w = min(window, g + 1) segments, oldest first.  phat_g = the first p with the largest A_g[p].

Tracking.  phi_0 = phat_0.  Later d = ((phat_g - phi_(g-1) + 12) mod 24) - 12 and phi_g moves one
sample towards phat_g (mod 24) if |d| >= 2, else stays: a dead band of one sample.

Symbols.  Segment g gives x[768 g + 24 j + phi_g] for j = j0 .. 31 (as they are, non-finite ones
included), j0 = 0 but 1 when phi stepped 23 -> 0 and -1 when it stepped 0 -> 23, so consecutive
symbol instants are 23, 24 or 25 samples apart and a wrap neither drops nor repeats a symbol.

Pairing.  Symbols have a global index m.  Over the pairs (m, m + 1) whose second symbol lies in
segment g, c0_g counts those with even m where (s[m] > 0) != (s[m + 1] > 0) and c1_g those with odd
m; C0, C1 are their sums over the last min(window, g + 1) segments.  Segment 0 sets pi = 0 if
C0 >= C1 else 1; later pi moves to the other parity only when that parity's count exceeds pi's by
more than `hysteresis`.  pi_g holds for the pairs whose second symbol lies in segment g.

Bits.  A pair (m, m + 1) with m = pi (mod 2) whose first symbol is not already the second of an
emitted pair gives bit = s[m] > s[m + 1]; diff = bit xor the previous bit, the very first bit
giving none.
"""
from __future__ import annotations

import numpy as np

SPS = 24                 # samples per symbol
SEG_SYMBOLS = 32
SEG = SPS * SEG_SYMBOLS  # 768
MAX_WINDOW = 16


def step_phi(phi: int, phat: int) -> int:
    """phi moved one sample towards phat across the shorter way round, or left inside the dead band"""
    d = ((phat - phi + 12) % 24) - 12
    if d >= 2:
        return (phi + 1) % 24
    if d <= -2:
        return (phi - 1) % 24
    return phi


class RdsSymbolClock:
    """Symbol clock recovery of one stream.  process(x) takes any number of float32 samples (0
    included) and returns the differential bits they complete, uint8; any split of a stream into
    calls gives the same bits.  `instants` is the last call's list of symbol sample indices (since
    reset), `symbol_values` their samples: for tests."""

    def __init__(self, window: int = 4, hysteresis: int = 8):
        if not 1 <= int(window) <= MAX_WINDOW:
            raise ValueError(f"window={window} outside [1, {MAX_WINDOW}]")
        if not 0 <= int(hysteresis) <= 1 << 20:
            raise ValueError(f"hysteresis={hysteresis} outside [0, {1 << 20}]")
        self.window, self.hysteresis = int(window), int(hysteresis)
        self.reset()

    def reset(self):
        self._tail = np.zeros(0, dtype=np.float32)     # the samples of the incomplete segment
        self._pre = np.zeros(SPS, dtype=np.float32)    # the 24 samples before it
        self._E, self._C = [], []                      # the last window - 1 energy and count vectors
        self.consumed = self.segments = 0
        self.phi = self.pi = 0
        self.symbols = self.bits = 0
        self.steps_forward = self.steps_back = self.wraps = self.pairing_changes = 0
        self._last = np.float32(0)                     # the last symbol and whether a pair has used it
        self._last_used = False
        self._prev_bit = None
        self.instants, self.symbol_values = [], []

    def state(self) -> tuple:
        """(consumed samples, segments, phi, pi, symbols, bits, steps forward, steps back, wraps,
        pairing changes); `bits` counts the Manchester bits, one more than the differential bits"""
        return (self.consumed, self.segments, self.phi, self.pi, self.symbols, self.bits, self.steps_forward,
                self.steps_back, self.wraps, self.pairing_changes)

    def process(self, x) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float32).ravel()
        row = np.concatenate([self._pre, self._tail, x])          # row[24 + i] = sample consumed + i
        G = (len(row) - SPS) // SEG
        out = []
        self.instants, self.symbol_values = [], []
        if G:
            sq = row[SPS:SPS + G * SEG].astype(np.float64)
            sq[~np.isfinite(sq)] = 0.0
            sq = (sq * sq).reshape(G, SEG_SYMBOLS, SPS)
            E = np.zeros((G, SPS))
            for j in range(SEG_SYMBOLS):
                E += sq[:, j, :]
        for g in range(G):
            self._segment(row, SPS + g * SEG, E[g], out)
        done = G * SEG
        self._pre = row[done:done + SPS].copy()
        self._tail = row[done + SPS:].copy()
        return np.array(out, dtype=np.uint8)

    def _segment(self, row, o, E, out):
        """the segment whose first sample is row[o]"""
        first = self.segments == 0
        # energy window, oldest first
        self._E = (self._E + [E])[-self.window:]
        A = self._E[0].copy()
        for e in self._E[1:]:
            A = A + e
        phat = int(np.argmax(A))                                   # the first maximum
        j0 = 0
        if first:
            self.phi = phat
        else:
            new = step_phi(self.phi, phat)
            if new != self.phi:
                up = new == (self.phi + 1) % 24
                self.steps_forward += up
                self.steps_back += not up
                if up and new == 0:
                    j0 = 1
                elif not up and new == 23:
                    j0 = -1
                self.wraps += j0 != 0
            self.phi = new
        idx = o + SPS * np.arange(j0, SEG_SYMBOLS) + self.phi
        s = row[idx]
        base = self.consumed - (o - SPS)                           # row index -> stream sample index, less 24
        self.instants += (idx - SPS + base).tolist()
        self.symbol_values += s.tolist()
        # sign changes by the parity of the pair's first symbol
        pos = np.concatenate([[self._last], s]) > 0
        change = pos[1:] != pos[:-1]
        m = self.symbols - 1 + np.arange(len(s))                   # the pairs' first symbols
        if self.symbols == 0:
            change[0] = False
        c = (int(np.count_nonzero(change & (m % 2 == 0))), int(np.count_nonzero(change & (m % 2 == 1))))
        self._C = (self._C + [c])[-self.window:]
        C0, C1 = sum(v[0] for v in self._C), sum(v[1] for v in self._C)
        if first:
            self.pi = 0 if C0 >= C1 else 1
        else:
            other = (C1 - C0) if self.pi == 0 else (C0 - C1)
            if other > self.hysteresis:
                self.pi ^= 1
                self.pairing_changes += 1
        # the pairs: each symbol in at most one
        last, used, pi = self._last, self._last_used, self.pi
        q = self.symbols
        for v in s:
            if q > 0 and (q - 1) % 2 == pi and not used:
                bit = int(last > v)
                if self._prev_bit is not None:
                    out.append(bit ^ self._prev_bit)
                self._prev_bit = bit
                self.bits += 1
                used = True
            else:
                used = False
            last = v
            q += 1
        self._last, self._last_used = last, used
        self.symbols = q
        self.segments += 1
        self.consumed += SEG
