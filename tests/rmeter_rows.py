"""What tests/test_rmeter_model.py (CPU) and tests/test_rmeter.py (GPU) share: the rows, the ragged
call lengths, and the comparison of a meter with the rule (rtsdr.RowMeterModel).

What is compared: every integer field, the peaks (as values: -0 equals +0), the histogram, the
carried window and windows() exactly; the float64 sums within the bound of any summation order.  A
float64 sum of n terms x_i taken in any order lies within n 2^-53 sum|x_i| of the exact sum (each of
the n - 1 additions rounds a partial sum that is at most sum|x_i| by at most 2^-53 of it), so two such
sums differ by at most n 2^-52 sum|x_i|; the squares are exact in float64 and non-negative, so sumsq
is within a relative n 2^-52.  The totals add one rounding per call to that, which the count n of
all samples so far covers.  The bound does not constrain the chunking."""
import numpy as np

STREAM = 50_000
CALLS = (1, 99, 100, 101, 4095, 4096, 4097, 8195)
RAGGED = CALLS + (STREAM - sum(CALLS),)
INT_FIELDS = ("n", "nonfinite", "over", "windows", "calls", "total_n", "total_nonfinite", "total_over", "total_windows",
              "empty_windows", "wcount")
PEAK_FIELDS = ("max", "min", "total_max", "total_min", "wmax", "wmin")
CARRIED = ("total_n", "total_nonfinite", "total_over", "total_windows", "empty_windows", "total_max", "total_min", "wcount", "wmax",
           "wmin")


def rows_of(S, n, seed=0, nonfinite=True):
    """(S, n) float32: a tone plus noise around a per-stream offset, a few samples beyond +-1; from 8
    samples on a NaN, both infinities and a NaN with a payload"""
    rng = np.random.default_rng([seed, S, n])
    t = np.arange(n)
    x = (0.4 * np.sin(2 * np.pi * t / 977.0 + np.arange(S)[:, None]) + 0.1 * rng.standard_normal((S, n))
         + 0.05 * np.arange(S)[:, None]).astype(np.float32)
    x[:, n // 3] = 1.5
    x[0, (2 * n) // 3] = -1.25
    if nonfinite and n >= 8:
        x[:, 5] = np.nan
        x[0, n - 3] = -np.inf
        x[S - 1, n // 2] = np.inf
        x.view(np.uint32)[S // 2, 2] = 0xffc00abc
    return x


class SumBound:
    """sum|x| and the count of the finite samples, of the latest call and of all calls"""

    def __init__(self, S):
        self.call_abs, self.total_abs = np.zeros(S), np.zeros(S)

    def take(self, x):
        d = np.where(np.isfinite(x), x, 0).astype(np.float64)
        self.call_abs = np.sum(np.abs(d), axis=1)
        self.total_abs = self.total_abs + self.call_abs


def check(got, want, bound, what=""):
    """got, want: (records, hist, windows) of a meter and of the rule after the same calls"""
    (gr, gh, gw), (wr, wh, ww) = got, want
    for k in INT_FIELDS:
        assert getattr(gr, k).dtype == np.int64 and np.array_equal(getattr(gr, k), getattr(wr, k)), (what, k, getattr(gr, k), getattr(wr, k))
    for k in PEAK_FIELDS:
        assert getattr(gr, k).dtype == np.float32 and np.array_equal(getattr(gr, k), getattr(wr, k)), (what, k, getattr(gr, k), getattr(wr, k))
    assert gh.dtype == np.uint64 and np.array_equal(gh, wh), (what, "hist")
    assert gw.dtype == np.float32 and gw.shape == ww.shape and np.array_equal(gw, ww), (what, "windows", gw.shape, ww.shape)
    eps = 2.0 ** -52
    for pre, n, ab in (("", wr.n, bound.call_abs), ("total_", wr.total_n, bound.total_abs)):
        g, w = getattr(gr, pre + "sum"), getattr(wr, pre + "sum")
        assert np.all(np.abs(g - w) <= n * eps * ab), (what, pre + "sum", g, w)
        g, w = getattr(gr, pre + "sumsq"), getattr(wr, pre + "sumsq")
        assert np.all(np.abs(g - w) <= n * eps * w), (what, pre + "sumsq", g, w)
