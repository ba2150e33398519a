"""What tests/test_sos.py (GPU) and tests/test_sos_model.py (CPU) share: the coefficient sets, the
rows, the references and the bound of a cascade of second-order sections (RowSos, csrc/sos.hip), and
the placement of rows between guards.

The bound, per sample of a row:   |y - y_ref| <= 2^-24 |y_ref| + 16 e_ref + 2^-50 G
and for the carried state:        |zf - zf_ref| <= 16 e_ref + 2^-50 G
  y_ref, zf_ref  scipy.signal.sosfilt in float64.
  G              max|x| prod_k ||h_k||_1, the section norms from 2^17-sample impulse responses: the
                 largest value any section's output can take, the scale rounding errors come in.
  e_ref          the largest difference, up to the sample in question, between sosfilt in float64 and
                 the same recursion run sample by sample in long double (64-bit mantissa) on the
                 same row: the reference's own rounding noise, computed here on the CPU and never
                 from the device.
  2^-24 |y_ref|  the one rounding of the row to float32.
Why 16: two summation orders of equal statistics differ by about sqrt(2) of that noise, a numpy model
of the kernels' structure with correctly rounded powers measured at most 3.1 x, and the device
contracts multiplies and adds differently again; a power table built in float64 by repeated squaring
misses the bound by 20-200 x on the sets with poles next to z = 1, a lost wave or tile carry by many
orders.

The long-double loop runs once for all sets together (the sets a vector, padded to four sections
with the identity) on rows of the longest length; every shorter length is a prefix of it, a filter
being causal."""
import functools

import numpy as np
from scipy import signal

TILE = 2048
LENGTHS = (1, 2, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 2 * 2048 + 3, 6149, 65 * 2048 + 1)
NMAX = max(LENGTHS)
S = 3
GUARD = np.float32(1e30)
PAD = 64                     # guard floats in front of the first row and behind the last

assert np.finfo(np.longdouble).eps < 2 ** -60, "the reference loop needs a 64-bit mantissa"


def coefficient_sets():
    kw = np.array([[1.53512485958697, -2.69169618940638, 1.19839281085285, 1.0, -1.69065929318241, 0.73248077421585],
                   [1.0, -2.0, 1.0, 1.0, -1.99004745483398, 0.99007225036621]])
    return {
        "k_weighting": kw,
        "notch": signal.tf2sos(*signal.iirnotch(19e3, 30, 48e3)),
        "ellip8": signal.ellip(8, 0.1, 80, 15e3, fs=48e3, output="sos"),
        "butter_hp20": signal.butter(2, 20, "hp", fs=48e3, output="sos"),
        "pole_near_minus_1": np.array([[0.5, -0.3, 0.1, 1.0, 1.8, 0.81]]),
    }


SETS = tuple(coefficient_sets())


def rows_of(n=NMAX, seed=7):
    """(S, n) float32: noise, a tone per row and an offset, about unit amplitude"""
    rng = np.random.default_rng([seed, S, n])
    t = np.arange(n)
    return (0.5 * rng.standard_normal((S, n)) + 0.4 * np.sin(2 * np.pi * t / 977.0 + np.arange(S)[:, None])
            + 0.1 * np.arange(S)[:, None]).astype(np.float32)


def gain_bound(sos, x):
    imp = np.zeros(1 << 17)
    imp[0] = 1.0
    g = float(np.max(np.abs(x)))
    for sec in np.atleast_2d(sos):
        g *= float(np.sum(np.abs(signal.sosfilt(sec[None, :], imp))))
    return g


def longdouble_loop(soses, x, checkpoints):
    """The recursion of sosfilt sample by sample in long double, for all the sets at once.
    Returns y [nsets, S, n] and {n: state [nsets, S, 4, 2]} at the checkpoints."""
    ld = np.longdouble
    ns, (rows, n) = len(soses), x.shape
    c = np.zeros((4, 6, ns, 1), dtype=ld)
    c[:, 0] = 1
    for i, sos in enumerate(soses):
        for k, sec in enumerate(sos):
            c[k, :, i, 0] = sec.astype(ld)
    b0, b1, b2, a1, a2 = c[:, 0], c[:, 1], c[:, 2], c[:, 4], c[:, 5]
    z1, z2 = np.zeros((4, ns, rows), dtype=ld), np.zeros((4, ns, rows), dtype=ld)
    xl = np.ascontiguousarray(x.astype(ld).T)
    y = np.empty((n, ns, rows), dtype=ld)
    states, marks = {}, set(checkpoints)
    for i in range(n):
        v = xl[i]
        for k in range(4):
            o = b0[k] * v + z1[k]
            z1[k] = b1[k] * v - a1[k] * o + z2[k]
            z2[k] = b2[k] * v - a2[k] * o
            v = o
        y[i] = v
        if i + 1 in marks:
            states[i + 1] = np.stack([z1, z2], axis=-1).transpose(1, 2, 0, 3).copy()
    return y.transpose(1, 2, 0), states


class Reference:
    """Of one coefficient set: the rows x, sosfilt's y64 [S, NMAX], the running e_ref [S, NMAX] (the
    noise up to each sample) and G; zf(n) and e_ref at a length."""

    def __init__(self, name, sos, x, y_ld):
        self.name, self.sos, self.x, self.K = name, sos, x, sos.shape[0]
        self.y64 = signal.sosfilt(sos, x.astype(np.float64), axis=-1)
        self.noise = np.maximum.accumulate(np.abs(self.y64.astype(np.longdouble) - y_ld).astype(np.float64), axis=1)
        self.G = gain_bound(sos, x)

    def zf(self, n, zi=None, start=0):
        """scipy's [S, K, 2] state after the samples [start, n) from zi"""
        z = np.zeros((self.K, S, 2)) if zi is None else np.ascontiguousarray(np.asarray(zi).transpose(1, 0, 2))
        return np.ascontiguousarray(signal.sosfilt(self.sos, self.x[:, start:n].astype(np.float64), axis=-1, zi=z)[1].transpose(1, 0, 2))

    def slack(self, n):
        """[S, n]: 16 e_ref + 2^-50 G for each sample of a call that ends at sample n"""
        return 16.0 * self.noise[:, :n] + 2.0 ** -50 * self.G

    def share_y(self, y, n, rows=slice(None)):
        """the largest |y - y_ref| / bound over the first n samples of the rows"""
        ref = self.y64[rows, :n]
        bound = 2.0 ** -24 * np.abs(ref) + self.slack(n)[rows]
        return float(np.max(np.abs(y.astype(np.float64) - ref) / bound))

    def share_beyond_rounding(self, y, n, rows=slice(None)):
        """what of |y - y_ref| the rounding to float32 does not explain, as a share of 16 e_ref + 2^-50 G (printed, not asserted)"""
        ref = self.y64[rows, :n]
        return float(np.max((np.abs(y.astype(np.float64) - ref) - 2.0 ** -24 * np.abs(ref)) / self.slack(n)[rows]).clip(0))

    def share_z(self, z, n, rows=slice(None)):
        bound = self.slack(n)[rows, -1][:, None, None]
        return float(np.max(np.abs(z - self.zf(n)[rows]) / bound))


@functools.lru_cache(maxsize=None)
def references():
    """{name: Reference}, computed once per session"""
    sets = coefficient_sets()
    x = rows_of()
    y_ld, _ = longdouble_loop(list(sets.values()), x, ())
    return {name: Reference(name, sos, x, y_ld[i]) for i, (name, sos) in enumerate(sets.items())}


class Rows:
    """One device allocation, reused by the calls of a test: rows placed `off` floats past a 16-byte
    boundary, `stride` floats apart, 1e30 before, between and after them."""

    def __init__(self, sdr, ctx, nfloats):
        self.nfloats = nfloats + 2 * PAD + 8
        self.buf = sdr.DeviceBuffer(ctx, 4 * self.nfloats)
        assert self.buf.ptr % 256 == 0

    def place(self, x, off=0, stride=None):
        """x [rows, n] (None entries: guards only, `rows` = x[0], n = x[1]); returns (ptr, stride)"""
        rows, n = x.shape
        stride = n if stride is None else stride
        self.host = np.full(PAD + off + rows * stride + PAD, GUARD, dtype=np.float32)
        assert self.host.size <= self.nfloats
        for s in range(rows):
            self.host[PAD + off + s * stride:PAD + off + s * stride + n] = x[s]
        self.buf.upload(self.host)
        self.geom = (off, stride, rows, n)
        return self.buf.ptr + 4 * (PAD + off), stride

    def guards(self, rows, n, off=0, stride=None):
        """only guards, for an output of [rows, n]"""
        return self.place(np.full((rows, n), GUARD, dtype=np.float32), off, stride)

    def fetch(self):
        """(rows [rows, n], everything else) as the device holds them now"""
        off, stride, rows, n = self.geom
        got = self.buf.download(self.host.size)
        mask = np.zeros(got.size, dtype=bool)
        for s in range(rows):
            mask[PAD + off + s * stride:PAD + off + s * stride + n] = True
        return got[mask].reshape(rows, n), got[~mask]

    def free(self):
        self.buf.free()
