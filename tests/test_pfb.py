"""The polyphase filter bank (sdr_pfb, csrc/pfb.hip; rtsdr.FilterBank): one IQ capture to the
selected bins of a uniform grid of M bins, each at Fs / D.  Parity is against the f64 definition
    y_c[m] = sum_j h[j] x[mD - j] exp(-2 pi i ((bin_c (k mod M)) mod M) / M),   k = pos + mD - j
with the phase in integer arithmetic: scipy.signal.lfilter(h, 1, x exp(-2 pi i phase))[::D].

Tolerance, the channelizer's (tests/test_ddc.py), with G = sum|h| max|x|:
    |y - y_ref| <= 1e-6 |y_ref| + 5e-7 G
test_arithmetic_emulation runs a numpy emulation of the kernel's arithmetic (the f32 fold as an
FMA chain over q, the f16 hi / lo split of u and of the DFT rows, f32 accumulation per 32-wide K
step, acc_c / 2048 + acc_h, the f32 rotation from the M-entry table) against it without a GPU."""
import ctypes

import numpy as np
import pytest
from scipy.signal import firwin, lfilter, resample_poly, upfirdn

WINDOW = 64          # output times per window (include/sdr.h SDR_PFB_WINDOW; 16 where the buffers exceed 80 KB of LDS)
LO = np.float32(2048.0)


# ---- the f64 reference ----------------------------------------------------------------------
def ubins(bins, M):
    return [int(b) % M for b in bins]


def ref_pfb(x, M, bins, h, D, pos=0, decimating=False):
    """x: complex128 samples at absolute indices pos, pos + 1, ...; zero before.  decimating:
    upfirdn computes only every D-th output of the same filter (the long-filter cases;
    test_reference_forms pins it to lfilter(.)[::D])"""
    km = (np.arange(len(x), dtype=np.int64) + int(pos)) % M
    rows = []
    for b in ubins(bins, M):
        z = x * np.exp(-2j * np.pi * ((b * km) % M) / M)
        rows.append(upfirdn(h, z, 1, D)[:len(x) // D] if decimating else lfilter(h, 1.0, z)[::D])
    return np.stack(rows)


def to_complex(iq, u8=False):
    v = (iq.astype(np.float64) - 128.0) / 128.0 if u8 else iq.astype(np.float64)
    return v[0::2] + 1j * v[1::2]


def interleave(z):
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=1).reshape(-1), dtype=np.float32)


def scale_g(h, x):
    return float(np.sum(np.abs(h)) * np.max(np.abs(x)))


def bound_of(ref, G):
    return 1e-6 * np.abs(ref) + 5e-7 * G


def check(y, ref, G, what=""):
    err = np.abs(y.astype(np.complex128) - ref)
    worst = float(np.max(err / bound_of(ref, G)))
    print(f"pfb {what}: max err {np.max(err):.3e} = {np.max(err) / G:.3e} G, {worst:.3f} of the bound")
    assert y.shape == ref.shape
    assert worst <= 1.0, (what, worst, float(np.max(err) / G))
    return float(np.max(err) / G)


def noise_iq(n, seed, u8=False):
    rng = np.random.default_rng(seed)
    if u8:
        return rng.integers(0, 256, 2 * n, dtype=np.uint8)
    return (0.5 * rng.standard_normal(2 * n)).astype(np.float32)


def tones_iq(n, M):
    """three tones at full scale: on a bin, between two bins, near the band edge"""
    k = np.arange(n)
    z = sum(a * np.exp(2j * np.pi * (nu * k + 0.1 * i)) for i, (a, nu) in enumerate(zip((1.0, 0.3, 0.5), (1.0 / M, 0.123456, -0.31))))
    return interleave(z)


def proto(M, T):
    return firwin(T, 1.0 / M) if (M > 1 and T > 1) else np.eye(1, T)[0]


# ---- CPU ------------------------------------------------------------------------------------
def test_pfb_coeffs(sdr):
    for M in (2, 12, 96):
        b = sdr.design.pfb_coeffs(M)
        assert len(b) == 8 * M and np.array_equal(b, firwin(8 * M, 1.0 / M))
    assert np.array_equal(sdr.design.pfb_coeffs(16, 3), firwin(48, 1.0 / 16))
    assert np.array_equal(sdr.design.pfb_coeffs(1), [1, 0, 0, 0, 0, 0, 0, 0])
    assert np.array_equal(sdr.design.pfb_coeffs(1, 1), [1.0])


def test_argument_errors_before_device_work(sdr):
    """Python raises ValueError before a context exists; the C entry point refuses the same
    arguments (SDR_EINVAL with a message naming the argument) before it looks at its context."""
    F = sdr.FilterBank
    h = firwin(16, 0.25)
    for kw in (dict(nbins=8, bins=[]), dict(nbins=0), dict(nbins=257), dict(nbins=8, bins=np.zeros(257, int)),
               dict(nbins=8, bins=[8]), dict(nbins=8, bins=[-5]), dict(nbins=8, bins=[1.5]), dict(nbins=8, decim=0),
               dict(nbins=8, decim=65), dict(nbins=8, taps=np.zeros(4097)), dict(nbins=8, taps=4097), dict(nbins=8, taps=0),
               dict(nbins=8, taps=np.r_[h, np.nan]), dict(nbins=8, iq_dtype=np.int16), dict(nbins=8, fs=0.0)):
        args = dict(dict(fs=1.0, decim=4), **kw)
        with pytest.raises(ValueError):
            F(**args)
    lib = sdr.load_library()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    out = ctypes.c_void_p()

    def create(nbins, nch, bins, b, decim, dtype=0, taps=None):
        k, t = np.asarray(bins, dtype=np.int32), np.asarray(b, dtype=np.float64)
        return lib.sdr_pfb_create(None, nbins, nch, k.ctypes.data_as(ip), t.ctypes.data_as(dp), len(t) if taps is None else taps,
                                  decim, dtype, ctypes.byref(out))
    for args, word in (((0, 1, [0], h, 4), "nbins"), ((257, 1, [0], h, 4), "nbins"), ((8, 0, [0], h, 4), "nch"),
                       ((8, 257, np.zeros(257), h, 4), "nch"), ((8, 1, [0], h, 0), "decim"), ((8, 1, [0], h, 65), "decim"),
                       ((8, 1, [0], h, 4, 0, 0), "taps"), ((8, 1, [0], h, 4, 0, 4097), "taps"), ((8, 2, [0, 8], h, 4), "bin[1]"),
                       ((8, 1, [-1], h, 4), "bin[0]"), ((8, 1, [0], np.r_[h, np.inf], 4), "finite"), ((8, 1, [0], h, 4, 2), "dtype"),
                       ((8, 1, [0], h, 4), "context is NULL")):
        assert create(*args) == -1 and word in lib.sdr_last_error().decode(), (args, lib.sdr_last_error())
    assert lib.sdr_pfb_create(None, 8, 1, None, None, 16, 4, 0, ctypes.byref(out)) == -1 and "NULL" in lib.sdr_last_error().decode()
    assert lib.sdr_pfb_create(None, 8, 1, None, None, 16, 4, 0, None) == -1 and "out" in lib.sdr_last_error().decode()
    assert lib.sdr_pfb_process_dev(None, None, 8, None, 8) == -1
    assert lib.sdr_pfb_run(None, None, 8, None, 8) == -1
    assert lib.sdr_pfb_reset(None, 0) == -1 and lib.sdr_pfb_position(None, None) == -1


def polyphase_f64(x, M, bins, h, D, pos):
    """the form the kernel uses, in f64"""
    T = len(h)
    P = -(-T // M)
    hp = np.r_[h, np.zeros(P * M - T)]
    xp = np.r_[np.zeros(P * M, np.complex128), x]
    Mo = len(x) // D
    p = np.arange(M)
    out = np.empty((len(bins), Mo), np.complex128)
    for m in range(Mo):
        u = sum(hp[p + q * M] * xp[P * M + m * D - p - q * M] for q in range(P))
        s = (pos + m * D) % M
        for c, b in enumerate(ubins(bins, M)):
            out[c, m] = np.exp(-2j * np.pi * ((b * s) % M) / M) * np.sum(np.exp(2j * np.pi * ((b * p) % M) / M) * u)
    return out


@pytest.mark.parametrize("M,D,T", [(12, 5, 36), (96, 8, 150)])
def test_reference_forms(M, D, T):
    """the polyphase identity in f64, and upfirdn as lfilter(.)[::D]"""
    n, pos = 40 * D, 12345 * D
    x = to_complex(noise_iq(n, 5))
    h = proto(M, T)
    bins = [0, 1, M // 2, M - 1, 5]
    ref = ref_pfb(x, M, bins, h, D, pos)
    G = scale_g(h, x)
    assert np.max(np.abs(polyphase_f64(x, M, bins, h, D, pos) - ref)) <= 1e-13 * G
    assert np.max(np.abs(ref_pfb(x, M, bins, h, D, pos, decimating=True) - ref)) <= 1e-13 * G


def split(v):
    v = v.astype(np.float32)
    hi = v.astype(np.float16).astype(np.float32)
    lo = ((v - hi) * LO).astype(np.float16).astype(np.float32)
    return hi, lo


def emulate(xf, M, bins, h, D, pos=0, drop_u_lo=False, f32_phase=False):
    """The kernel's arithmetic in numpy.  The fold: per (output time, p) an f32 FMA chain over q
    (the product exact in f64, the sum rounded once to f32).  u (Re, Im interleaved, K = 2M
    padded to 32 KS) and the DFT rows split into f16 hi / lo; each 32-wide K step's products
    summed (f64, rounded once: the MFMA's internal order is not modelled) into an f32
    accumulator, the cross terms into a second one; y = acc_c / 2048 + acc_h; then the rotation
    by the f32 table entry of t = (bin ((pos + mD) mod M)) mod M, an f32 complex multiply.
    drop_u_lo / f32_phase: the two defects the bound must see."""
    T = len(h)
    P = -(-T // M)
    PM = P * M
    KS = (2 * M + 31) // 32
    K = 32 * KS
    n = len(xf) // 2
    Mo = n // D
    h32 = np.r_[h, np.zeros(PM - T)].astype(np.float32).astype(np.float64)
    xr = np.r_[np.zeros(PM, np.float32), xf[0::2].astype(np.float32)].astype(np.float64)
    xi = np.r_[np.zeros(PM, np.float32), xf[1::2].astype(np.float32)].astype(np.float64)
    p = np.arange(M)
    at = PM + D * np.arange(Mo)[:, None] - p[None, :]                              # [Mo][M]: x[mD - p]
    ur = np.zeros((Mo, M), np.float32)
    ui = np.zeros((Mo, M), np.float32)
    for q in range(P):
        hq = h32[p + q * M][None, :]
        ur = (hq * xr[at - q * M] + ur.astype(np.float64)).astype(np.float32)
        ui = (hq * xi[at - q * M] + ui.astype(np.float64)).astype(np.float32)
    U = np.zeros((K, Mo), np.float32)
    U[0:2 * M:2] = ur.T
    U[1:2 * M:2] = ui.T
    bh, bl = split(U)
    if drop_u_lo:
        bl = np.zeros_like(bl)
    t = np.arange(M)
    rot = (np.cos(2 * np.pi * t / M).astype(np.float32), (-np.sin(2 * np.pi * t / M)).astype(np.float32))
    s = (pos + D * np.arange(Mo, dtype=np.int64)) % M
    out = np.empty((len(bins), Mo), np.complex64)
    for c, b in enumerate(ubins(bins, M)):
        th = 2 * np.pi * ((b * p) % M) / M
        A = np.zeros((2, K))
        A[0, 0:2 * M:2], A[0, 1:2 * M:2], A[1, 0:2 * M:2], A[1, 1:2 * M:2] = np.cos(th), -np.sin(th), np.sin(th), np.cos(th)
        ah, al = split(A.astype(np.float32))
        acc_h = np.zeros((2, Mo), np.float32)
        acc_c = np.zeros((2, Mo), np.float32)
        for st in range(KS):
            sl = slice(32 * st, 32 * st + 32)
            f = lambda a, b_: a[:, sl].astype(np.float64) @ b_[sl].astype(np.float64)   # noqa: E731
            acc_h = (acc_h + f(ah, bh).astype(np.float32)).astype(np.float32)
            acc_c = (acc_c + f(ah, bl).astype(np.float32)).astype(np.float32)
            acc_c = (acc_c + f(al, bh).astype(np.float32)).astype(np.float32)
        y = (acc_c.astype(np.float64) / 2048.0 + acc_h).astype(np.float32)
        if f32_phase:      # the defect: bin (pos + mD) in f32, never reduced mod M, to half turns
            k32 = (pos + D * np.arange(Mo, dtype=np.int64)).astype(np.float32)
            ht = ((np.float32(b) * k32).astype(np.float32) * np.float32(2.0 / M)).astype(np.float32).astype(np.float64)
            rx, ry = np.cos(np.pi * ht).astype(np.float32), (-np.sin(np.pi * ht)).astype(np.float32)
        else:
            tt = (b * s) % M
            rx, ry = rot[0][tt], rot[1][tt]
        y64 = y.astype(np.float64)
        re = ((y[0] * rx).astype(np.float32).astype(np.float64) - y64[1] * ry).astype(np.float32)
        im = ((y[1] * rx).astype(np.float32).astype(np.float64) + y64[0] * ry).astype(np.float32)
        out[c] = re + 1j * im
    return out


def emu_bins(M):
    return sorted(set(ubins([0, 1, M // 2, M - 1, 5, -3], M)))


@pytest.mark.parametrize("M,D,T", [(7, 3, 5), (12, 5, 36), (64, 8, 256), (96, 8, 768), (16, 4, 256)])
@pytest.mark.parametrize("kind", ["noise", "tones"])
def test_arithmetic_emulation(M, D, T, kind):
    Mo, pos = 60, 12345 * D
    n = Mo * D
    xf = noise_iq(n, 11) if kind == "noise" else tones_iq(n, M)
    h = proto(M, T)
    x = to_complex(xf)
    bins = emu_bins(M)
    ref = ref_pfb(x, M, bins, h, D, pos)
    e = check(emulate(xf, M, bins, h, D, pos), ref, scale_g(h, x), f"emulation {kind} M={M} D={D} T={T}")
    assert e < 2e-7


def test_emulation_sees_a_dropped_lo_plane_and_an_unreduced_phase():
    """the bound is tight enough to catch the defects it is meant for (more than 10 x the bound):
    u without its lo plane, and a rotation from bin (pos + mD) in f32 without the reduction mod M
    (at a position past 2^31, where an f32 no longer holds the sample index)"""
    M, D, T, Mo = 64, 8, 256, 60
    pos = (1 << 31) + 12345 * D
    xf = tones_iq(Mo * D, M)
    h = proto(M, T)
    x = to_complex(xf)
    G = scale_g(h, x)
    bins = [1, 5, 31, 63]
    ref = ref_pfb(x, M, bins, h, D, pos)
    check(emulate(xf, M, bins, h, D, pos), ref, G, "emulation, no defect")
    for kw in (dict(drop_u_lo=True), dict(f32_phase=True)):
        err = np.abs(emulate(xf, M, bins, h, D, pos, **kw) - ref)
        assert np.max(err / bound_of(ref, G)) > 10.0, (kw, float(np.max(err / bound_of(ref, G))))


# ---- GPU ------------------------------------------------------------------------------------
def up16(v):
    return (v + 15) // 16 * 16


def plan(M, nch, T, D):
    """csrc/pfb.hip's choice of window and of where the DFT rows live: (outputs per window, A in LDS)"""
    KS, NT, PM = (2 * M + 31) // 32, (nch + 7) // 8, -(-T // M) * M

    def lds(W):
        return up16(8 * M) + up16(32 * NT) + up16(4 * PM) + up16(8 * ((W - 1) * D + PM)) + 2 * W * (32 * KS + 8) * 2
    W = WINDOW if lds(WINDOW) <= 80 * 1024 else 16
    return W, lds(W) + NT * KS * 2048 <= 65536


def run(sdr, M, bins, h, D, iq, calls=None, dtype=np.float32, pos=None):
    fb = sdr.FilterBank(M, 1.0, D, bins=bins, taps=h, iq_dtype=dtype)
    try:
        if pos is not None:
            fb.reset(pos)
        calls = calls or [len(iq) // 2]
        assert sum(calls) == len(iq) // 2
        out, at = [], 0
        for n in calls:
            out.append(fb.process(iq[2 * at:2 * (at + n)]))
            at += n
        return np.concatenate(out, axis=1)
    finally:
        fb.close()


MID_M, MID_D, MID_T = 12, 5, 36


@pytest.mark.gpu
@pytest.mark.parametrize("k0", [0, 1, 4, 5, 11, 12, 35, 36])     # 0, 1, D - 1, D, M - 1, M, T - 1, T
def test_impulse(sdr, gpu_ctx, k0):
    M, D, T, n = MID_M, MID_D, MID_T, 5 * 20
    bins = (0, 1, 6, 11)
    h = proto(M, T)
    a = 1 + 0.5j
    x = np.zeros(n, np.complex128)
    x[k0] = a
    y = run(sdr, M, bins, h, D, interleave(x))
    m = np.arange(n // D)
    j = m * D - k0
    taps = np.where((j >= 0) & (j < T), h[np.clip(j, 0, T - 1)], 0.0)
    for c, b in enumerate(bins):
        exp = taps * a * np.exp(-2j * np.pi * b * k0 / M)
        assert np.max(np.abs(y[c] - exp)) <= 5e-7 * np.sum(np.abs(h)) * abs(a), (c, k0)
    check(y, ref_pfb(x, M, bins, h, D), scale_g(h, x), f"impulse k0={k0}")


def first(pred, values):
    return next(v for v in values if pred(v))


# the first M (T = 3M, D = 5, all bins) whose window is the smaller one, and the one before it;
# the first channel count at M = 32 whose DFT rows no longer fit the LDS, and the one before it
M_SMALL = first(lambda M: plan(M, M, 3 * M, MID_D)[0] == 16, range(1, 257))
NCH_L2 = first(lambda c: not plan(32, c, 96, MID_D)[1], range(1, 257))
MID = dict(M=MID_M, D=MID_D, T=MID_T, nch=None, count=WINDOW + 1)
SHAPES = ([dict(MID, M=v, T=min(4096, 3 * v)) for v in sorted({1, 2, 7, 16, 17, 96, 255, 256, M_SMALL - 1, M_SMALL})] +
          [dict(MID, M=32, T=96, nch=v) for v in (1, 7, 8, 9, 16, 17, NCH_L2 - 1, NCH_L2)] +
          [dict(MID, T=v) for v in (1, 11, 12, 13, 41)] +
          [dict(MID, M=256, D=64, T=4096), dict(MID, M=256, T=768, count=3 * 16 + 5)] +
          [dict(MID, D=v) for v in (1, 11, 12, 13, 64)] +
          [dict(MID, count=v) for v in (1, 15, 16, 17, WINDOW - 1, WINDOW, 3 * WINDOW + 5)])


def test_the_plan_names_both_windows_and_both_paths():
    assert 96 < M_SMALL <= 256 and plan(96, 96, 768, 8) == (WINDOW, False) and plan(M_SMALL - 1, M_SMALL - 1, 3 * M_SMALL - 3, MID_D) == (WINDOW, False)
    assert 17 < NCH_L2 <= 256 and plan(32, NCH_L2 - 1, 96, MID_D) == (WINDOW, True)
    assert plan(MID_M, MID_M, MID_T, MID_D) == (WINDOW, True) and plan(256, 256, 4096, 64) == (16, False)


@pytest.mark.gpu
@pytest.mark.parametrize("s", SHAPES, ids=lambda s: f"M{s['M']}-c{s['nch']}-T{s['T']}-D{s['D']}-m{s['count']}")
def test_shapes(sdr, gpu_ctx, s):
    M, D, T, Mo = s["M"], s["D"], s["T"], s["count"]
    bins = np.arange(M) if s["nch"] is None else (np.arange(s["nch"]) * 7 + 3) % M      # (repeats beyond M channels)
    h = proto(M, T)
    iq = noise_iq(Mo * D, 100 + M + T + D + Mo)
    x = to_complex(iq)
    check(run(sdr, M, bins, h, D, iq), ref_pfb(x, M, bins, h, D, decimating=T > 1024), scale_g(h, x), str(s))


@pytest.mark.gpu
@pytest.mark.parametrize("pos", [0, 12345 * 5])
def test_bins(sdr, gpu_ctx, pos):
    M, D, T, Mo = MID_M, MID_D, MID_T, 2 * WINDOW + 9
    bins = [0, 6, 11, -1, 5, -6, 5, 3]                 # M / 2 as 6 and -6, M - 1 as 11 and -1, 5 twice
    h = proto(M, T)
    iq = noise_iq(Mo * D, 21)
    x = to_complex(iq)
    y = run(sdr, M, bins, h, D, iq, pos=pos)
    check(y, ref_pfb(x, M, bins, h, D, pos), scale_g(h, x), f"bins pos={pos}")
    bits = y.view(np.uint32)
    assert np.array_equal(bits[4], bits[6]) and np.array_equal(bits[1], bits[5]) and np.array_equal(bits[2], bits[3])
    # rows of the GEMM are independent: channel 11 of 16 is the 1-bin object's row
    many = list((np.arange(16) * 5 + 2) % 32)
    many[11] = 9
    h32 = proto(32, 96)
    a = run(sdr, 32, [9], h32, D, iq, pos=pos)
    b = run(sdr, 32, many, h32, D, iq, pos=pos)
    assert np.array_equal(a[0].view(np.uint32), b[11].view(np.uint32))


@pytest.mark.gpu
def test_tones(sdr, gpu_ctx):
    M, D, T, Mo = 16, 4, 128, 4 * WINDOW + 3
    bins, amps = (1, 5, -4), (1.0, 0.3, 0.5)
    k = np.arange(Mo * D)
    z = sum(a * np.exp(2j * np.pi * ((b % M) / M * k + 0.1 * i)) for i, (a, b) in enumerate(zip(amps, bins)))
    iq = interleave(z)
    h = proto(M, T)
    x = to_complex(iq)
    y = run(sdr, M, bins, h, D, iq)
    check(y, ref_pfb(x, M, bins, h, D), scale_g(h, x), "tones")
    for c, a in enumerate(amps):      # each row settles on its own tone at DC, the others rejected
        assert abs(np.abs(np.mean(y[c, 2 * T // D:])) - a) < 0.02


@pytest.mark.gpu
@pytest.mark.parametrize("pos", [(1 << 31) + 12345 * 8, (1 << 32) - 8 * 8, 1 << 40])
def test_position(sdr, gpu_ctx, pos):
    M, D, T = MID_M, 8, MID_T                          # (decim 8: the positions are multiples of it)
    n = 32 * D
    bins = (1, 5, 6, 11)
    h = proto(M, T)
    iq = noise_iq(n, 41)
    x = to_complex(iq)
    fb = sdr.FilterBank(M, 1.0, D, bins=bins, taps=h)
    fb.reset(pos)
    y = np.concatenate([fb.process(iq[:n]), fb.process(iq[n:])], axis=1)       # two calls of 16 D
    assert fb.position == pos + n
    fb.close()
    check(y, ref_pfb(x, M, bins, h, D, pos), scale_g(h, x), f"position {pos}")


def splits(total, D, seed):
    rng = np.random.default_rng(seed)
    out = []
    while total:
        n = min(total, D * int(rng.integers(1, 40)))
        out.append(n)
        total -= n
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_carried_state(sdr, gpu_ctx, u8):
    M, D, T = MID_M, MID_D, MID_T
    n = 640 * D
    bins = (1, 6, 11)
    h = proto(M, T)
    dt = np.uint8 if u8 else np.float32
    iq = noise_iq(n, 31, u8)
    x = to_complex(iq, u8)
    ref, G = ref_pfb(x, M, bins, h, D), scale_g(h, x)
    cases = {"one": [n], "byD": [D] * (n // D), "by7D": [7 * D] * (n // (7 * D)) + ([n % (7 * D)] if n % (7 * D) else []),
             "uneven": splits(n, D, 4), "short_first": [2 * D, n - 2 * D]}       # (2 D = 10 < T - 1 = 35)
    ys = {k: run(sdr, M, bins, h, D, iq, calls=v, dtype=dt) for k, v in cases.items()}
    for k, y in ys.items():
        check(y, ref, G, f"carried {k} u8={u8}")
        assert np.all(np.abs(y - ys["one"]) <= 2 * bound_of(ref, G)), k
    fb = sdr.FilterBank(M, 1.0, D, bins=bins, taps=h, iq_dtype=dt)
    first_call = fb.process(iq[:2 * 24 * D])
    fb.process(iq[2 * 24 * D:])
    assert fb.position == n
    fb.reset(0)
    assert fb.position == 0
    again = fb.process(iq[:2 * 24 * D])
    assert np.array_equal(first_call.view(np.uint32), again.view(np.uint32))
    fb.close()


@pytest.mark.gpu
def test_u8_middle_setting(sdr, gpu_ctx):
    M, D, T, Mo = MID_M, MID_D, MID_T, WINDOW + 1
    h = proto(M, T)
    iq = noise_iq(Mo * D, 51, u8=True)
    x = to_complex(iq, True)
    bins = np.arange(M)
    check(run(sdr, M, bins, h, D, iq, dtype=np.uint8), ref_pfb(x, M, bins, h, D), scale_g(h, x), "u8 middle")
    y = run(sdr, M, bins, h, D, iq, calls=[D, 3 * D, (Mo - 4) * D], dtype=np.uint8)      # an odd split
    check(y, ref_pfb(x, M, bins, h, D), scale_g(h, x), "u8 split")


@pytest.mark.gpu
@pytest.mark.parametrize("T", [36, 37])
@pytest.mark.parametrize("shift", [0, 2])
def test_u8_byte_alignment(sdr, gpu_ctx, T, shift):
    """u8 samples start at any even byte: a device pointer 0 / 2 bytes past an aligned one, two
    calls (the second starts inside the buffer), an even and an odd history length"""
    M, D, Mo, bins = MID_M, MID_D, 2 * WINDOW + 3, (1, 6, 11)
    nch, n = len(bins), Mo * D
    h = proto(M, T)
    iq = noise_iq(n, 71, u8=True)
    x = to_complex(iq, True)
    buf = sdr.DeviceBuffer(gpu_ctx, 2 * n + 16)
    buf.upload(iq, offset=shift)
    out = sdr.DeviceBuffer(gpu_ctx, nch * Mo * 8)
    fb = sdr.FilterBank(M, 1.0, D, bins=bins, taps=h, iq_dtype=np.uint8, ctx=gpu_ctx)
    half = (Mo // 2) * D
    fb.process_dev(buf.ptr + shift, half, out.ptr, Mo)
    fb.process_dev(buf.ptr + shift + 2 * half, n - half, out.ptr + 8 * (Mo // 2), Mo)
    gpu_ctx.synchronize()
    y = out.download(nch * Mo * 2, np.float32).view(np.complex64).reshape(nch, Mo)
    check(y, ref_pfb(x, M, bins, h, D), scale_g(h, x), f"u8 alignment T={T} shift={shift}")
    with pytest.raises(ValueError):
        fb.process_dev(buf.ptr + 1, n, out.ptr, Mo)      # an odd address: not a whole complex sample
    fb.close()
    buf.free()
    out.free()


@pytest.mark.gpu
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_run_equals_process_dev_and_strides(sdr, gpu_ctx, u8):
    M, D, T, Mo, bins = MID_M, MID_D, MID_T, 2 * WINDOW + 7, (0, 1, 6, -1, 5)
    nch, n, stride = len(bins), Mo * D, Mo + 9
    h = proto(M, T)
    iq = noise_iq(n, 61, u8)
    lib = gpu_ctx.lib
    fb = sdr.FilterBank(M, 2.4e6, D, bins=bins, taps=h, iq_dtype=np.uint8 if u8 else np.float32, ctx=gpu_ctx)
    packed = fb.process(iq)
    host = np.full((nch, stride), np.complex64(7 - 3j))
    fb.reset(0)
    assert lib.sdr_pfb_run(fb.handle, iq.ctypes.data, n, host.ctypes.data, stride) == 0
    assert np.array_equal(host[:, :Mo].view(np.uint32), packed.view(np.uint32))
    assert np.all(host[:, Mo:] == np.complex64(7 - 3j))
    poison = np.full(nch * stride * 2 + 16, 0xABABABAB, np.uint32)
    din = sdr.DeviceBuffer.from_array(gpu_ctx, iq)
    dout = sdr.DeviceBuffer.from_array(gpu_ctx, poison)
    fb.reset(0)
    fb.process_dev(din.ptr, n, dout.ptr, stride)
    gpu_ctx.synchronize()
    got = dout.download(len(poison), np.uint32)
    rows = got[:nch * stride * 2].reshape(nch, 2 * stride)
    assert np.array_equal(rows[:, :2 * Mo], packed.view(np.uint32))
    assert np.all(rows[:, 2 * Mo:] == 0xABABABAB) and np.all(got[nch * stride * 2:] == 0xABABABAB)
    assert fb.position == n
    # call-time argument errors: refused before any launch, the position unchanged
    for args in ((din.ptr, n - 1, dout.ptr, stride), (din.ptr, 0, dout.ptr, stride), (din.ptr, n, dout.ptr, Mo - 1)):
        with pytest.raises(ValueError):
            fb.process_dev(*args)
        assert lib.sdr_pfb_process_dev(fb.handle, *args) == -1
    with pytest.raises(ValueError):
        fb.process(iq[:2 * (D + 1)])
    for bad in (-5, 3):
        with pytest.raises(ValueError):
            fb.reset(bad)
    assert fb.position == n
    assert np.array_equal(fb.bins, [0, 1, 6, 11, 5])
    assert np.array_equal(fb.freqs_hz, np.array([0, 1, -6, -1, 5]) / 12 * 2.4e6)
    din.free()
    dout.free()
    fb.close()


@pytest.mark.gpu
def test_against_the_channelizer(sdr, gpu_ctx):
    """bin / 64 cycles per sample is exact in the channelizer's 32-bit phase, so both objects
    follow the same definition: rows within twice the bound of each other"""
    M, D, T, Mo = 64, 8, 256, 3 * WINDOW + 5
    pos = 12345 * D
    bins = np.array([0, 1, 2, 5, 9, 17, 30, 31, -32, -31, -20, -9, -3, -2, -1, 13])
    h = proto(M, T)
    iq = noise_iq(Mo * D, 81)
    x = to_complex(iq)
    ref, G = ref_pfb(x, M, bins, h, D, pos), scale_g(h, x)
    y = run(sdr, M, bins, h, D, iq, pos=pos)
    check(y, ref, G, "against the channelizer: the filter bank")
    ch = sdr.Channelizer(bins / 64.0, 1.0, D, taps=h, ctx=gpu_ctx)
    ch.reset(pos)
    z = ch.process(iq)
    ch.close()
    check(z, ref, G, "against the channelizer: the channelizer")
    assert np.all(np.abs(y - z) <= 2 * bound_of(ref, G))


@pytest.mark.gpu
def test_into_the_receiver(sdr, gpu_ctx):
    """capture -> filter bank -> receiver without leaving HBM, against the f64 reference's rows
    (rounded to f32) through an identically configured receiver.  Bound 2e-5 on the audio, as
    tests/test_ddc.py::test_into_the_receiver: a relative IQ error eps moves the arctan demod by
    <= 2 eps rad, the audio filter's sum|b| is below 3, and eps <= 1.5e-6 G / amplitude here."""
    B, UP, nst, M = 51200, 8, 3, 16
    bins = (-4, 1, 5)
    n_nb = 2 * B
    n = n_nb * UP
    k = np.arange(n)
    wide = np.zeros(n, np.complex128)
    for s, (b, snr) in enumerate(zip(bins, (30.0, 20.0, 25.0))):
        st = sdr.synth.fm_iq(n_nb, seed=s + 1, snr_db=snr).astype(np.float64)
        z = resample_poly(st[0::2] + 1j * st[1::2], UP, 1)                # zero-stuff x8 and low-pass
        wide += z * np.exp(2j * np.pi * ((b % M) / M) * k)
    wide *= 0.3
    iq = interleave(wide)
    h = sdr.design.pfb_coeffs(M)
    assert len(h) == 128
    stride = (n_nb + 31) // 32 * 32
    fb = sdr.FilterBank(M, 1.0, UP, bins=bins, taps=h, ctx=gpu_ctx)
    din = sdr.DeviceBuffer.from_array(gpu_ctx, iq)
    rows = sdr.DeviceBuffer(gpu_ctx, nst * stride * 8)
    fb.process_dev(din.ptr, n, rows.ptr, stride)
    ref = ref_pfb(to_complex(iq), M, bins, h, UP, decimating=True).astype(np.complex64)
    ref_rows = np.zeros((nst, stride), np.complex64)
    ref_rows[:, :n_nb] = ref
    dref = sdr.DeviceBuffer.from_array(gpu_ctx, ref_rows)
    audio = []
    for buf in (rows, dref):
        rx = sdr.Receiver(nst, B, iq_dtype=np.float32, ctx=gpu_ctx)
        blocks = []
        for blk in range(2):
            rx.process_dev(buf.ptr + 8 * B * blk, stride)
            blocks.append(rx.output("audio"))
        audio.append(np.concatenate(blocks, axis=1))
        rx.close()
    a, b = audio
    err = float(np.max(np.abs(a - b)))
    print(f"pfb into the receiver: audio max |a - b| = {err:.3e} (audio peak {np.max(np.abs(b)):.3f})")
    assert a.shape == (nst, 2 * (B // 10 // 5)) and np.all(np.isfinite(a))
    assert err <= 2e-5, err
    for i in range(nst):
        for j in range(i + 1, nst):
            assert np.max(np.abs(a[i] - a[j])) > 1e-2, (i, j)           # no swapped or repeated row
    for d in (din, rows, dref):
        d.free()
    fb.close()
