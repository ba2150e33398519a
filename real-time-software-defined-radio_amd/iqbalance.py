"""IQ imbalance and DC offset correction of a capture on the host, pure numpy f64 (no GPU, no libsdr).

IqBalance is the specification of the device stage (IqCorrector, csrc/iqc.hip): one block of a
capture (interleaved float32 IQ, or uint8 as (x - 128) / 128) -> the same block as interleaved
float32 with the front end's DC offset removed and the Q branch's gain and phase error undone.

A sum of stations away from 0 Hz is a proper complex signal: E[z^2] = 0, so I and Q have equal power
and are uncorrelated.  What the capture's second moments show beyond that is the front end's doing,
and one 2 x 2 real matrix undoes it: a Gram-Schmidt step on the five moments.  The estimate is blind
(no pilot, no calibration tone) and frequency-independent: one matrix for the whole band.

State.  The smoothed raw moments m = (mI, mQ, pII, pQQ, pIQ); the coefficients (dI, dQ, c1, c2),
initially (0, 0, 0, 1); the counters updates, skipped, holds.

A call of n >= 1 complex samples with `estimate` on:

1. Block moments.  r = (sum I, sum Q, sum I^2, sum Q^2, sum I Q) / n, the samples widened to f64 (a
   product of two float32 values is exact in f64): each of the five is one sum divided once by n.
2. Smoothing.  If any of the five is not finite: skipped += 1 and nothing else changes.  Otherwise
   m = r on the first update and m = m + rate (r - m) on later ones (rate in (0, 1], default 0.125: a
   design default, not a measurement), then updates += 1.
3. Coefficients from m.  A = pII - mI mI, B = pQQ - mQ mQ, C = pIQ - mI mQ, t = B - (C / A) C.  Valid
   iff A > 0, t > 0 and both finite: then c2 = sqrt(A / t), c1 = -(C / A) c2, dI = mI, dQ = mQ.
   Otherwise the previous coefficients stay and holds += 1 (an all-zero block, a constant block,
   Q = I).  With dc off dI = dQ = 0 are installed (the moments stay central); with balance off
   c1 = 0, c2 = 1.
4. The same block is mapped with the coefficients just computed:
   I' = float32(I - dI), Q' = float32(c1 (I - dI) + c2 (Q - dQ)), evaluated in f64 as written (two
   products, one sum, no fused multiply-add) and rounded to float32 once.  A NaN sample stays a NaN
   at that sample only.

With `estimate` off, steps 1-3 are skipped.  set() installs coefficients (a front end calibrated
once), reset() returns to the initial state.

impropriety = ((A - B)^2 + 4 C^2) / (A + B)^2 of the smoothed moments is |E[z^2]|^2 / E[|z|^2]^2 of
the capture with its mean removed; for a small imbalance a quarter of it is the image's power over
the station's: image_db = 10 log10(impropriety / 4).
"""
from __future__ import annotations

import collections
import math

import numpy as np

NSTATE = 12                      # include/sdr.h SDR_IQC_NSTATE
DEFAULT_RATE = 0.125

IqState = collections.namedtuple(
    "IqState", "mI mQ pII pQQ pIQ dI dQ c1 c2 updates skipped holds impropriety image_db")


def check_rate(rate) -> float:
    rate = float(rate)
    if not (math.isfinite(rate) and 0.0 < rate <= 1.0):
        raise ValueError(f"rate={rate} outside (0, 1]")
    return rate


def check_coeffs(coeff):
    c = tuple(float(v) for v in coeff)
    if len(c) != 4 or not all(math.isfinite(v) for v in c):
        raise ValueError("coefficients: four finite values dI, dQ, c1, c2")
    return c


def central_moments(m):
    """A, B, C of step 3 from the five raw moments (f64, the operations as written)."""
    mI, mQ, pII, pQQ, pIQ = (np.float64(v) for v in m)
    return pII - mI * mI, pQQ - mQ * mQ, pIQ - mI * mQ


def coefficients(m, dc=True, balance=True):
    """Step 3: (dI, dQ, c1, c2) from the five raw moments, or None where they are not valid."""
    with np.errstate(all="ignore"):
        A, B, C = central_moments(m)
        q = C / A
        t = B - q * C
        if not (A > 0 and t > 0 and np.isfinite(A) and np.isfinite(t)):
            return None
        c2 = np.sqrt(A / t)
        c1 = -q * c2
    return (float(m[0]) if dc else 0.0, float(m[1]) if dc else 0.0, float(c1) if balance else 0.0, float(c2) if balance else 1.0)


def impropriety(m) -> float:
    """((A - B)^2 + 4 C^2) / (A + B)^2 of the five raw moments (NaN before the first update)."""
    with np.errstate(all="ignore"):
        A, B, C = central_moments(m)
        return float(((A - B) * (A - B) + 4.0 * C * C) / ((A + B) * (A + B)))


def make_state(raw) -> IqState:
    """The 12 values of sdr_iqc_state plus impropriety and image_db."""
    raw = [float(v) for v in raw]
    imp = impropriety(raw[:5]) if raw[9] > 0 else float("nan")
    with np.errstate(all="ignore"):
        db = float(10.0 * np.log10(np.float64(imp) / 4.0))
    return IqState(*raw[:9], int(raw[9]), int(raw[10]), int(raw[11]), imp, db)


def as_f64_pairs(iq, u8: bool):
    """A host block as (I, Q) in f64: interleaved float32 / uint8, or complex for a float32 object."""
    iq = np.asarray(iq)
    if np.iscomplexobj(iq):
        if u8:
            raise ValueError("a uint8 corrector takes interleaved uint8 IQ")
        iq = np.ascontiguousarray(iq, dtype=np.complex64).view(np.float32)
    iq = np.ascontiguousarray(iq, dtype=np.uint8 if u8 else np.float32)
    if iq.ndim != 1 or iq.size % 2 or iq.size < 2:
        raise ValueError("expected a 1-D array of interleaved I, Q values, at least one pair")
    x = iq.astype(np.float64)
    if u8:
        x = (x - 128.0) / 128.0
    return x[0::2], x[1::2]


class IqBalance:
    """The rule of the module's docstring on one capture stream."""

    def __init__(self, iq_dtype=np.float32, rate: float = DEFAULT_RATE, dc: bool = True, balance: bool = True):
        dt = np.dtype(iq_dtype)
        if dt not in (np.dtype(np.float32), np.dtype(np.uint8)):
            raise ValueError(f"iq_dtype {dt}: float32 or uint8")
        self.u8 = dt == np.uint8
        self.rate, self.dc, self.balance = check_rate(rate), bool(dc), bool(balance)
        self.reset()

    def reset(self):
        self.m = np.zeros(5)
        self.coeff = (0.0, 0.0, 0.0, 1.0)
        self.updates = self.skipped = self.holds = 0

    def set(self, dI: float, dQ: float, c1: float, c2: float):
        self.coeff = check_coeffs((dI, dQ, c1, c2))

    def state(self) -> IqState:
        return make_state([*self.m, *self.coeff, self.updates, self.skipped, self.holds])

    @property
    def impropriety(self) -> float:
        return self.state().impropriety

    @property
    def image_db(self) -> float:
        return self.state().image_db

    def _estimate(self, I, Q):
        n = float(len(I))
        with np.errstate(all="ignore"):
            r = np.array([np.sum(I) / n, np.sum(Q) / n, np.sum(I * I) / n, np.sum(Q * Q) / n, np.sum(I * Q) / n])
        if not np.all(np.isfinite(r)):
            self.skipped += 1
            return
        self.m = r if self.updates == 0 else self.m + self.rate * (r - self.m)
        self.updates += 1
        c = coefficients(self.m, self.dc, self.balance)
        if c is None:
            self.holds += 1
        else:
            self.coeff = c

    def process(self, iq, estimate: bool = True) -> np.ndarray:
        """One block -> the corrected block, interleaved float32 (2 n values)."""
        I, Q = as_f64_pairs(iq, self.u8)
        if estimate:
            self._estimate(I, Q)
        return apply(I, Q, self.coeff)


def apply(I, Q, coeff) -> np.ndarray:
    """Step 4 with the given (dI, dQ, c1, c2) on f64 I, Q: interleaved float32."""
    dI, dQ, c1, c2 = (np.float64(v) for v in coeff)
    out = np.empty(2 * len(I), dtype=np.float32)
    with np.errstate(all="ignore"):
        x = I - dI
        y = Q - dQ
        out[0::2] = x
        out[1::2] = c1 * x + c2 * y
    return out
