"""Synthetic (rrc_i, rrc_q) rows for the carrier-phase tests (tests/test_rds_carrier_model.py on the
CPU, tests/test_rds_carrier.py on the GPU): a noiseless row x of tests/rds_clock_rows.py turned by a
carrier phase theta(t) = theta0 + drift t (degrees, degrees/s, t in seconds at 57 kHz), with
independent white noise sigma on each branch:

    i = float32(x cos theta + N(0, sigma)),  q = float32(x sin theta + N(0, sigma))

both drawn from default_rng(seed + 7), i's noise first."""
import functools

import numpy as np

import rds_clock_rows as rc

FS = 57_000.0


@functools.lru_cache(maxsize=None)
def _pair(theta0, drift, ppm, sigma, seed, groups):
    x = rc.row(ppm=ppm, sigma=0.0, seed=seed, groups=groups).astype(np.float64)
    n = len(x)
    th = np.deg2rad(theta0 + drift * np.arange(n) / FS)
    rng = np.random.default_rng(seed + 7)
    i = (x * np.cos(th) + rng.normal(0.0, sigma, n)).astype(np.float32)
    q = (x * np.sin(th) + rng.normal(0.0, sigma, n)).astype(np.float32)
    i.setflags(write=False)
    q.setflags(write=False)
    return i, q


def pair(theta0=0.0, drift=0.0, ppm=0.0, sigma=0.05, seed=0, groups=rc.GROUPS):
    """A read-only (i, q) pair of float32 rows (cached)."""
    return _pair(float(theta0), float(drift), float(ppm), float(sigma), int(seed), int(groups))


def model_calls(sdr, i, q, cuts, **kw):
    """the model over the cuts of one pair: per call (y, state, moments, kappas)"""
    m = sdr.RdsCarrierPhase(**kw)
    out, o = [], 0
    for n in cuts:
        y = m.process(i[o:o + n], q[o:o + n])
        out.append((y, m.state(), m.moments(), list(m.kappas)))
        o += n
    return out


def carrier_blocks(sdr, i, q, seed, groups=rc.GROUPS, **kw):
    """generator blocks through RdsCarrierPhase, RdsSymbolClock and RdsBlockSync"""
    return rc.clock_blocks(sdr, sdr.RdsCarrierPhase(**kw).process(i, q), seed, groups)
