"""The row resampler (sdr_rsmp, csrc/rsmp.hip; rtsdr.RowResampler): N rows of device memory,
complex or real, resampled by up / down.  Parity is against the f64 polyphase definition
    y[m] = sum_{q < P} g[r + q U] x[s - q],   g = U h zero-padded to P U,   m D = s U + r
(= U lfilter(h, 1, zero-stuff(x, U))[::D]; test_reference_forms pins it to scipy's upfirdn and
resample_poly), x zero before the stream start.

Tolerance, the channelizer's (tests/test_ddc.py), per real component:
    |y - y_ref| <= 1e-6 |y_ref| + 5e-7 G,   G = U max_r sum_q |h[r + q U]| max|x|
Any split of a stream into calls must give the bits of one call."""
import ctypes

import numpy as np
import pytest
from scipy.signal import firwin, resample_poly, upfirdn

TILE = 2048          # outputs a workgroup produces as a unit (include/sdr.h SDR_RSMP_TILE)


# ---- the f64 reference ----------------------------------------------------------------------
def padded(h, U):
    P = -(-len(h) // U)
    return np.r_[np.asarray(h, np.float64), np.zeros(P * U - len(h))], P


def ref_rsmp(x, h, U, D, m=None):
    """x: (rows, n) f64 or complex128, zero before index 0; the outputs m (all n U / D of them
    when None), in f64"""
    hp, P = padded(h, U)
    g = U * hp
    x = np.atleast_2d(x)
    n = x.shape[1]
    m = np.arange(n * U // D, dtype=np.int64) if m is None else np.asarray(m, dtype=np.int64)
    s, r = (m * D) // U, (m * D) % U
    xp = np.concatenate([np.zeros((x.shape[0], P - 1), x.dtype), x], axis=1)
    y = np.zeros((x.shape[0], len(m)), x.dtype)
    for q in range(P):
        y += g[r + q * U][None, :] * xp[:, s - q + P - 1]
    return y


def scale_g(h, U, x):
    hp, P = padded(h, U)
    return float(U * np.max(np.sum(np.abs(hp.reshape(P, U)), axis=0)) * np.max(np.abs(parts(x))))


def parts(v):
    """the real components of an array, complex or real, as f64"""
    v = np.asarray(v)
    return np.stack([v.real, v.imag]).astype(np.float64) if np.iscomplexobj(v) else v.astype(np.float64)


def share(y, ref, G):
    """the worst error as a share of the bound, per real component"""
    a, b = parts(y), parts(ref)
    return float(np.max(np.abs(a - b) / (1e-6 * np.abs(b) + 5e-7 * G)))


def check(y, ref, G, what=""):
    assert y.shape == ref.shape, (what, y.shape, ref.shape)
    worst = share(y, ref, G)
    print(f"rsmp {what}: max err {np.max(np.abs(parts(y) - parts(ref))) / G:.3e} G, {worst:.3f} of the bound")
    assert worst <= 1.0, (what, worst)
    return worst


def noise(rows, n, seed, cplx):
    rng = np.random.default_rng(seed)
    if cplx:
        return (0.5 * (rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n)))).astype(np.complex64)
    return (0.5 * rng.standard_normal((rows, n))).astype(np.float32)


def wide(x):
    return x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)


def taps_of(U, D, T):
    """T taps of the default design's kind (a half-band filter where the rate does not change);
    one tap is 1 / U, so that g is 1.0"""
    if T == 1:
        return np.array([1.0 / U])
    return firwin(T, 1.0 / max(U, D, 2), window=("kaiser", 5.0))


def call_len(U, D, outputs):
    """the smallest legal n that gives at least `outputs` outputs per row"""
    g = int(np.gcd(U, D))
    return -(-outputs // (U // g)) * (D // g)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- CPU ------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,D", [(24, 25), (3, 4), (147, 160)])
def test_reference_forms(sdr, U, D):
    h = sdr.design.resample_coeffs(U, D)
    assert np.array_equal(h, firwin(20 * D + 1, 1.0 / D, window=("kaiser", 5.0)))
    n = call_len(U, D, 700)
    x = wide(noise(2, n, 3, True))
    ref = ref_rsmp(x, h, U, D)
    G = scale_g(h, U, x)
    for row in range(2):
        assert np.max(np.abs(ref[row] - U * upfirdn(h, x[row], U, D)[:ref.shape[1]])) <= 1e-12 * G
        poly = resample_poly(x[row], U, D)
        assert len(poly) == ref.shape[1]
        assert np.max(np.abs(ref[row, 10:] - poly[:-10])) <= 1e-12 * G


def test_resample_coeffs(sdr):
    rc = sdr.design.resample_coeffs
    kaiser = ("kaiser", 5.0)
    assert np.array_equal(rc(24, 25), firwin(501, 1 / 25, window=kaiser))
    assert np.array_equal(rc(160, 147, taps=None), firwin(3201, 1 / 160, window=kaiser))
    assert np.array_equal(rc(1024, 1023), firwin(4096, 1 / 1024, window=kaiser))       # cut to the longest filter
    assert np.array_equal(rc(3, 25, 77), firwin(77, 1 / 25, window=kaiser))
    with pytest.raises(ValueError):
        rc(0, 5)


def test_argument_errors_before_device_work(sdr):
    """Python raises ValueError before a context exists; the C entry point refuses the same
    arguments (SDR_EINVAL with a message naming the argument) before it looks at its context."""
    R = sdr.RowResampler
    assert (R.TILE, R.MAX_FACTOR, R.MAX_TAPS, R.MAX_PHASE_TAPS, R.MAX_ROWS) == (TILE, 1024, 4096, 256, 65535)
    h = firwin(16, 0.25)
    for kw in (dict(nrows=0), dict(nrows=65536), dict(up=0), dict(up=1025), dict(down=0), dict(down=1025), dict(taps=0),
               dict(taps=4097), dict(taps=np.zeros(4097)), dict(taps=np.zeros(0)), dict(taps=np.r_[h, np.nan]),
               dict(taps=np.r_[h, np.inf]), dict(up=1, taps=257), dict(up=2, taps=np.ones(513)), dict(taps=np.ones((2, 4)))):
        args = dict(dict(nrows=3, up=3, down=2), **kw)
        with pytest.raises(ValueError):
            R(**args)
    lib = sdr.load_library()
    dp = ctypes.POINTER(ctypes.c_double)
    out = ctypes.c_void_p()

    def create(nrows, elems, b, up, down, taps=None):
        t = np.asarray(b, dtype=np.float64)
        return lib.sdr_rsmp_create(None, nrows, elems, t.ctypes.data_as(dp), len(t) if taps is None else taps, up, down,
                                   ctypes.byref(out))
    for args, word in (((0, 2, h, 3, 2), "nrows"), ((65536, 2, h, 3, 2), "nrows"), ((3, 0, h, 3, 2), "elems"),
                       ((3, 3, h, 3, 2), "elems"), ((3, 2, h, 0, 2), "up"), ((3, 2, h, 1025, 2), "up"), ((3, 2, h, 3, 0), "down"),
                       ((3, 2, h, 3, 1025), "down"), ((3, 2, h, 3, 2, 0), "taps"), ((3, 2, h, 3, 2, 4097), "taps"),
                       ((3, 1, np.ones(257), 1, 2), "taps"), ((3, 2, np.r_[h, np.inf], 3, 2), "finite"),
                       ((3, 2, np.r_[np.nan, h], 3, 2), "finite"), ((3, 2, h, 3, 2), "context is NULL")):
        assert create(*args) == -1 and word in lib.sdr_last_error().decode(), (args, lib.sdr_last_error())
    assert lib.sdr_rsmp_create(None, 3, 2, None, 16, 3, 2, ctypes.byref(out)) == -1 and "NULL" in lib.sdr_last_error().decode()
    assert lib.sdr_rsmp_create(None, 3, 2, None, 16, 3, 2, None) == -1 and "out" in lib.sdr_last_error().decode()
    assert lib.sdr_rsmp_process_dev(None, None, 8, 8, None, 12) == -1
    assert lib.sdr_rsmp_run(None, None, 8, 8, None, 12) == -1
    assert lib.sdr_rsmp_reset(None) == -1 and lib.sdr_rsmp_position(None, None) == -1


# ---- GPU ------------------------------------------------------------------------------------
class Dev:
    """rows of a resampler in device memory: the input uploaded once, calls at any offsets"""

    def __init__(self, sdr, ctx, rs, x, in_stride=None, out_stride=None, in_off=0, out_off=0, pad=0):
        self.sdr, self.ctx, self.rs = sdr, ctx, rs
        self.rows, self.n = x.shape
        self.es = 8 if rs.complex else 4
        self.mo = self.n * rs.up // rs.down
        self.in_stride = in_stride or self.n
        self.out_stride = out_stride or self.mo
        self.in_off, self.out_off = in_off, out_off           # samples past the allocation's start
        self.dt = np.complex64 if rs.complex else np.float32
        host = np.full(in_off + self.rows * self.in_stride + pad, np.nan, self.dt)
        rows_view = host[in_off:in_off + self.rows * self.in_stride].reshape(self.rows, self.in_stride)
        rows_view[:, :self.n] = x
        self.din = sdr.DeviceBuffer.from_array(ctx, host)
        self.nout = 2 * (out_off + self.rows * self.out_stride + pad) if rs.complex else out_off + self.rows * self.out_stride + pad
        self.dout = sdr.DeviceBuffer.from_array(ctx, np.full(self.nout, 0xABABABAB, np.uint32))

    @property
    def in_ptr(self):
        return self.din.ptr + self.es * self.in_off

    @property
    def out_ptr(self):
        return self.dout.ptr + self.es * self.out_off

    def run(self, calls=None):
        at = 0
        for n in calls or [self.n]:
            self.rs.process_dev(self.in_ptr + self.es * at, n, self.in_stride,
                                self.out_ptr + self.es * (at * self.rs.up // self.rs.down), self.out_stride)
            at += n
        assert at == self.n
        return self.result()

    def raw(self):
        self.ctx.synchronize()
        return self.dout.download(self.nout, np.uint32)

    def result(self):
        w = self.es // 4
        got = self.raw()[w * self.out_off:w * (self.out_off + self.rows * self.out_stride)]
        return got.reshape(self.rows, w * self.out_stride)[:, :w * self.mo].copy().view(self.dt)

    def free(self):
        self.din.free()
        self.dout.free()


PARITY = [(1, 1, 1), (1, 1, 2), (2, 1, 33), (1, 3, 31), (3, 2, 4), (5, 3, 4), (24, 25, 501), (3, 25, 501), (147, 160, 3201),
          (160, 147, 3201), (16, 15, 4096), (1, 1, 256)]


@pytest.mark.gpu
@pytest.mark.parametrize("cplx", [True, False], ids=["complex", "real"])
@pytest.mark.parametrize("U,D,T", PARITY, ids=lambda v: str(v))
def test_parity(sdr, gpu_ctx, U, D, T, cplx):
    n = call_len(U, D, 2 * TILE + 3)
    h = taps_of(U, D, T)
    x = noise(3, n, 1000 + U + D + T, cplx)
    rs = sdr.RowResampler(3, U, D, taps=h, complex=cplx, ctx=gpu_ctx)
    y = rs.process(x)
    assert rs.position == n
    rs.close()
    check(y, ref_rsmp(wide(x), h, U, D), scale_g(h, U, x), f"parity {U}/{D} T={T} {'complex' if cplx else 'real'}")
    if (U, D, T) == (1, 1, 1):
        assert np.array_equal(bits(y), bits(x))        # one tap of 1.0 copies the bits


def uneven(total, step, seed):
    rng = np.random.default_rng(seed)
    out = []
    while total:
        n = min(total, step * int(rng.integers(1, 40)))
        out.append(n)
        total -= n
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cplx", [True, False], ids=["complex", "real"])
@pytest.mark.parametrize("U,D,T", [(2, 1, 33), (1, 3, 31), (24, 25, 501), (147, 160, 3201)], ids=lambda v: str(v))
def test_carried_state(sdr, gpu_ctx, U, D, T, cplx):
    step = D // int(np.gcd(U, D))
    n = call_len(U, D, 2 * TILE + 3)
    P = -(-T // U)
    h = taps_of(U, D, T)
    x = noise(3, n, 2000 + U + D, cplx)
    ref, G = ref_rsmp(wide(x), h, U, D), scale_g(h, U, x)
    rs = sdr.RowResampler(3, U, D, taps=h, complex=cplx, ctx=gpu_ctx)
    dev = Dev(sdr, gpu_ctx, rs, x)
    one = dev.run()
    assert rs.position == n
    check(one, ref, G, f"carried {U}/{D} one call")
    whole, rest = divmod(n, 7 * step)
    cases = {"by_step": [step] * (n // step), "by_7_steps": [7 * step] * whole + ([rest] if rest else []),
             "uneven": uneven(n, step, 4)}
    if U * D <= 3:
        assert P - 1 > step                            # these two carry more history than a minimal call brings
    for name, calls in cases.items():
        rs.reset()
        assert rs.position == 0
        y = dev.run(calls)
        assert rs.position == n
        assert np.array_equal(bits(y), bits(one)), (name, share(y, ref, G))
    rs.reset()
    first = call_len(U, D, TILE // 2)
    again = dev.run([first, n - first])
    assert np.array_equal(bits(again), bits(one))
    rs.close()
    dev.free()


@pytest.mark.gpu
@pytest.mark.parametrize("cplx", [True, False], ids=["complex", "real"])
def test_strides_and_untouched_memory(sdr, gpu_ctx, cplx):
    U, D, T, rows = 24, 25, 501, 5
    n = call_len(U, D, 2 * TILE + 3)
    mo = n * U // D
    step = D
    h = taps_of(U, D, T)
    x = noise(rows, n, 31, cplx)
    lib = gpu_ctx.lib
    rs = sdr.RowResampler(rows, U, D, taps=h, complex=cplx, ctx=gpu_ctx)
    packed = rs.process(x)
    check(packed, ref_rsmp(wide(x), h, U, D), scale_g(h, U, x), "strides, packed")
    in_stride, out_stride, w = n + 5, mo + 7, 2 if cplx else 1
    # device rows: NaN between the input rows and behind them, a pattern between and behind the output rows
    dev = Dev(sdr, gpu_ctx, rs, x, in_stride=in_stride, out_stride=out_stride, pad=16)
    rs.reset()
    y = dev.run()
    assert np.array_equal(bits(y), bits(packed))
    got = dev.raw()
    grid = got[:w * rows * out_stride].reshape(rows, w * out_stride)
    assert np.all(grid[:, w * mo:] == 0xABABABAB) and np.all(got[w * rows * out_stride:] == 0xABABABAB)
    # sdr_rsmp_run with strides: the same bits, the host gaps intact
    hin = np.full((rows, in_stride), np.nan, x.dtype)
    hin[:, :n] = x
    hout = np.full((rows, w * out_stride), 0xABABABAB, np.uint32)
    rs.reset()
    assert lib.sdr_rsmp_run(rs.handle, hin.ctypes.data, n, in_stride, hout.ctypes.data, out_stride) == 0
    assert np.array_equal(hout[:, :w * mo], bits(packed)) and np.all(hout[:, w * mo:] == 0xABABABAB)
    assert rs.position == n
    # call-time errors: refused before any launch, from Python and from C, the position unchanged
    es = dev.es
    inside = dev.in_ptr + es * (in_stride * (rows - 1) + n - 1)          # out begins on in's last sample
    for args in ((dev.in_ptr, n - 1, in_stride, dev.out_ptr, out_stride), (dev.in_ptr, 0, in_stride, dev.out_ptr, out_stride),
                 (dev.in_ptr, n, n - 1, dev.out_ptr, out_stride), (dev.in_ptr, n, in_stride, dev.out_ptr, mo - 1),
                 (dev.in_ptr + es // 2, n, in_stride, dev.out_ptr, out_stride),
                 (dev.in_ptr, n, in_stride, dev.out_ptr + es // 2, out_stride),
                 (dev.in_ptr, n, in_stride, inside, out_stride), (dev.in_ptr, n, in_stride, dev.in_ptr - es * step, out_stride),
                 (0, n, in_stride, dev.out_ptr, out_stride), (dev.in_ptr, n, in_stride, 0, out_stride)):
        with pytest.raises(ValueError):
            rs.process_dev(*args)
        assert lib.sdr_rsmp_process_dev(rs.handle, *args) == -1, args
        assert rs.position == n
    with pytest.raises(ValueError):
        rs.process(x[:, :n - 1])
    with pytest.raises(ValueError):
        rs.process(x[:2])
    assert rs.position == n
    # the history is unchanged too: the stream goes on as if nothing had been refused
    x2 = noise(rows, step * 4, 32, cplx)
    tail = rs.process(x2)
    both = ref_rsmp(wide(np.concatenate([x, x2], axis=1)), h, U, D)
    check(tail, both[:, mo:], scale_g(h, U, np.concatenate([x, x2], axis=1)), "strides, the call after the refused ones")
    rs.close()
    dev.free()


@pytest.mark.gpu
@pytest.mark.parametrize("cplx,shift", [(True, 1), (False, 1), (False, 2), (False, 3)], ids=lambda v: str(v))
def test_alignment(sdr, gpu_ctx, cplx, shift):
    """rows that start `shift` samples past a 16-byte boundary, in and out; odd strides, so that
    the rows of one call differ in alignment as well"""
    U, D, T = 24, 25, 501
    n = call_len(U, D, 2 * TILE + 3)
    mo = n * U // D
    h = taps_of(U, D, T)
    x = noise(3, n, 41, cplx)
    rs = sdr.RowResampler(3, U, D, taps=h, complex=cplx, ctx=gpu_ctx)
    aligned = Dev(sdr, gpu_ctx, rs, x, in_stride=-(-n // 4) * 4, out_stride=-(-mo // 4) * 4)
    assert aligned.in_ptr % 16 == 0 and aligned.out_ptr % 16 == 0
    a = aligned.run()
    check(a, ref_rsmp(wide(x), h, U, D), scale_g(h, U, x), f"alignment, aligned {'complex' if cplx else 'real'}")
    rs.reset()
    moved = Dev(sdr, gpu_ctx, rs, x, in_stride=n + 9, out_stride=mo + 7, in_off=shift, out_off=shift)
    assert moved.in_ptr % 16 == shift * moved.es and moved.out_ptr % 16 == shift * moved.es
    b = moved.run()
    assert np.array_equal(bits(a), bits(b))
    w = moved.es // 4
    got = moved.raw()
    assert np.all(got[:w * shift] == 0xABABABAB)
    assert np.all(got[w * shift:].reshape(3, w * (mo + 7))[:, w * mo:] == 0xABABABAB)
    rs.close()
    aligned.free()
    moved.free()


@pytest.mark.gpu
def test_offsets_beyond_32_bits(sdr, gpu_ctx):
    """m D passes 2^32 inside one call: real, one row, 1024 / 1023, 4096 taps"""
    U, D, T = 1024, 1023, 4096
    n = D * 4200
    mo = U * 4200
    h = sdr.design.resample_coeffs(U, D)
    assert len(h) == T and (mo - 1) * D > 1 << 32
    x = noise(1, n, 51, False)
    rs = sdr.RowResampler(1, U, D, complex=False, ctx=gpu_ctx)
    assert np.array_equal(rs.taps, h)
    y = rs.process(x)
    rs.close()
    assert y.shape == (1, mo)
    mid = (1 << 32) // D
    m = np.r_[np.arange(4096), np.arange(mid - 2048, mid + 2048), np.arange(mo - 4096, mo)]
    assert m[4096 + 2048] * D <= 1 << 32 < m[4096 + 2049] * D
    check(y[:, m], ref_rsmp(wide(x), h, U, D, m), scale_g(h, U, x), "offsets beyond 32 bits")


@pytest.mark.gpu
@pytest.mark.parametrize("cplx", [True, False], ids=["complex", "real"])
def test_non_finite_containment(sdr, gpu_ctx, cplx):
    U, D, T = 24, 25, 501
    P = -(-T // U)
    n = call_len(U, D, 2 * TILE + 3)
    h = taps_of(U, D, T)
    clean = noise(3, n, 61, cplx)
    x = clean.copy()
    at = (1000, 3 * n // 4)
    x[1, at[0]] = np.nan
    x[1, at[1]] = np.inf
    rs = sdr.RowResampler(3, U, D, taps=h, complex=cplx, ctx=gpu_ctx)
    y = rs.process(x)
    rs.close()
    zeroed = clean.copy()
    zeroed[1, list(at)] = 0
    ref, G = ref_rsmp(wide(zeroed), h, U, D), scale_g(h, U, clean)
    m = np.arange(y.shape[1], dtype=np.int64)
    s = (m * D) // U
    in_window = np.zeros(len(m), bool)
    on_a_tap = np.zeros(len(m), bool)
    for k in at:
        in_window |= (s - P + 1 <= k) & (k <= s)
        j = m * D - k * U
        on_a_tap |= (j >= 0) & (j < T) & (h[np.clip(j, 0, T - 1)] != 0)
    assert np.all(in_window[on_a_tap]) and on_a_tap.sum() >= 2 * (P - 1)
    assert np.all(np.isfinite(parts(y[[0, 2]]))) and np.all(np.isfinite(parts(y[1, ~in_window])))
    check(y[[0, 2]], ref[[0, 2]], G, "non-finite: the other rows")
    check(y[1:2, ~in_window], ref[1:2, ~in_window], G, "non-finite: its row, outside the windows")
    hit = parts(y[1, on_a_tap])
    assert not np.any(np.isfinite(hit if not cplx else hit[0]))        # (the complex sample's real part was set)


@pytest.mark.gpu
def test_into_the_receiver(sdr, gpu_ctx):
    """2.5 MS/s rows -> x 24/25 -> receiver at 2.4 MS/s without leaving HBM, against the f64
    reference's rows (rounded to f32) through an identically configured receiver.  Bound 2e-5 on
    the audio, tests/test_ddc.py::test_into_the_receiver's: a relative IQ error eps moves the
    arctan demod by <= 2 eps rad, the audio filter's sum|b| is below 3, and eps <= 1.5e-6 G /
    amplitude here."""
    U, D, nst, blocks = 24, 25, 3, 2
    n_in, B = 160000, 153600
    rows = np.empty((nst, blocks * n_in), np.complex64)
    # synth.fm_iq's stations carry the same programme: they differ in their noise and RDS symbols
    # only, so the SNRs are spread until every pair of audio rows is 1.7e-2 apart or more in the
    # f64 model of this chain (20 and 25 dB: 9e-3)
    for s, snr in enumerate((30.0, 10.0, 16.0)):
        st = sdr.synth.fm_iq(blocks * n_in, seed=s + 1, fs=2.5e6, snr_db=snr)
        rows[s] = (st[0::2] + 1j * st[1::2]).astype(np.complex64)
    rs = sdr.RowResampler(nst, U, D, ctx=gpu_ctx)
    assert len(rs.taps) == 501
    din = sdr.DeviceBuffer.from_array(gpu_ctx, rows)
    stride = blocks * B
    dout = sdr.DeviceBuffer(gpu_ctx, nst * stride * 8)
    ref = ref_rsmp(wide(rows), rs.taps, U, D).astype(np.complex64)
    assert ref.shape == (nst, stride)
    dref = sdr.DeviceBuffer.from_array(gpu_ctx, ref)
    audio = []
    for use_ref in (False, True):
        rx = sdr.Receiver(nst, B, iq_dtype=np.float32, ctx=gpu_ctx)
        got = []
        for blk in range(blocks):
            if use_ref:
                rx.process_dev(dref.ptr + 8 * B * blk, stride)
            else:
                rs.process_dev(din.ptr + 8 * n_in * blk, n_in, blocks * n_in, dout.ptr + 8 * B * blk, stride)
                rx.process_dev(dout.ptr + 8 * B * blk, stride)
            got.append(rx.output("audio"))
        audio.append(np.concatenate(got, axis=1))
        rx.close()
    a, b = audio
    err = float(np.max(np.abs(a - b)))
    print(f"rsmp into the receiver: audio max |a - b| = {err:.3e} (audio peak {np.max(np.abs(b)):.3f})")
    assert a.shape == (nst, blocks * (B // 10 // 5)) and np.all(np.isfinite(a))
    assert err <= 2e-5, err
    for i in range(nst):
        for j in range(i + 1, nst):
            assert np.max(np.abs(a[i] - a[j])) > 1e-2, (i, j)           # no swapped or repeated row
    for d in (din, dout, dref):
        d.free()
    rs.close()
