"""The wideband channelizer (sdr_ddc, csrc/ddc.hip; rtsdr.Channelizer): one IQ capture to nch
rows at Fs / D.  The reference has no channelizer, so parity is against the f64 definition
here: the integer phase phi_c(k) = ((inc_c k) mod 2^32) / 2^32 in uint64 arithmetic, then
scipy.signal.lfilter(h, 1, x exp(-2 pi i phi))[::D].

Tolerance, with G = sum|h| max|x| (the input-side scale a GEMM's rounding follows):
    |y - y_ref| <= 1e-6 |y_ref| + 5e-7 G
test_arithmetic_emulation runs a numpy emulation of the kernel's exact arithmetic (f16 hi / lo
splits of taps and samples, f32 accumulation per 32-wide K step, the 24-bit signed-turn phase,
f32 sin / cos, f32 complex multiply) against it without a GPU."""
import ctypes

import numpy as np
import pytest
from scipy.signal import firwin, lfilter, resample_poly

WINDOW = 64          # outputs per wave window (include/sdr.h SDR_DDC_WINDOW; 16 for the largest decimations)
LO = np.float32(2048.0)


# ---- the f64 reference ----------------------------------------------------------------------
def phase_inc(nu):
    return int(np.rint(nu * 4294967296.0)) % (1 << 32)


def phase_turns(inc, k):
    """((inc k) mod 2^32) / 2^32 for absolute indices k (uint64; the product wraps mod 2^64)"""
    return ((np.uint64(inc) * k.astype(np.uint64)) & np.uint64(0xFFFFFFFF)).astype(np.float64) / 4294967296.0


def ref_ddc(x, nus, h, D, pos=0):
    """x: complex128 samples at absolute indices pos, pos + 1, ...; zero before"""
    k = np.arange(len(x), dtype=np.uint64) + np.uint64(pos)
    return np.stack([lfilter(h, 1.0, x * np.exp(-2j * np.pi * phase_turns(phase_inc(nu), k)))[::D] for nu in nus])


def to_complex(iq, u8=False):
    v = (iq.astype(np.float64) - 128.0) / 128.0 if u8 else iq.astype(np.float64)
    return v[0::2] + 1j * v[1::2]


def scale_g(h, x):
    return float(np.sum(np.abs(h)) * np.max(np.abs(x)))


def check(y, ref, G, what=""):
    err = np.abs(y.astype(np.complex128) - ref)
    bound = 1e-6 * np.abs(ref) + 5e-7 * G
    worst = float(np.max(err / bound))
    print(f"ddc {what}: max err {np.max(err):.3e} = {np.max(err) / G:.3e} G, {worst:.3f} of the bound")
    assert y.shape == ref.shape
    assert worst <= 1.0, (what, worst, float(np.max(err) / G))
    return float(np.max(err) / G)


def noise_iq(n, seed, u8=False):
    rng = np.random.default_rng(seed)
    if u8:
        return rng.integers(0, 256, 2 * n, dtype=np.uint8)
    return (0.5 * rng.standard_normal(2 * n)).astype(np.float32)


def lowpass(T, D):
    return firwin(T, 1.0 / D if D > 1 else 0.5) if T > 1 else np.ones(1)


def nus_for(nch, seed=7):
    return np.random.default_rng(seed).uniform(-0.5, 0.5, nch)


# ---- CPU ------------------------------------------------------------------------------------
def test_channel_coeffs(sdr):
    for D in (2, 8, 10):
        b = sdr.design.channel_coeffs(D)
        assert len(b) == 8 * D and np.array_equal(b, firwin(8 * D, 1.0 / D))
    assert np.array_equal(sdr.design.channel_coeffs(8, 33), firwin(33, 1.0 / 8))
    assert np.array_equal(sdr.design.channel_coeffs(1, 5), [1, 0, 0, 0, 0])


def test_frequency_quantisation(sdr):
    inc, act = sdr.design.ddc_phase_inc, sdr.design.ddc_actual_freq
    assert inc(0.0) == 0 and act(0) == 0.0
    assert inc(0.5) == 1 << 31 and inc(-0.5) == 1 << 31 and act(1 << 31) == -0.5
    assert inc(1 / 3) == 1431655765 and act(inc(1 / 3)) == 1431655765 / 2.0 ** 32
    assert inc(-0.31) == (1 << 32) - int(np.rint(0.31 * 2.0 ** 32)) and act(inc(-0.31)) == -int(np.rint(0.31 * 2.0 ** 32)) / 2.0 ** 32
    assert inc(2.0 ** -32) == 1 and inc(-2.0 ** -32) == (1 << 32) - 1 and act((1 << 32) - 1) == -2.0 ** -32
    for nu in (0.0, 0.5, -0.5, 1 / 3, -0.31, 0.123456):
        assert inc(nu) == phase_inc(nu)
        assert abs(act(inc(nu)) - nu) <= 2.0 ** -33 or nu == 0.5          # (+0.5 is reported as -0.5)
    for bad in (0.5000001, -0.6, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            inc(bad)


def test_argument_errors_before_device_work(sdr):
    """Python raises ValueError before a context exists; the C entry point refuses the same
    arguments (SDR_EINVAL with a message) before it looks at its context."""
    C = sdr.Channelizer
    h = firwin(16, 0.25)
    for kw in (dict(freqs_hz=[], fs=1.0, decim=4), dict(freqs_hz=np.zeros(65), fs=1.0, decim=4),
               dict(freqs_hz=[0.1], fs=1.0, decim=0), dict(freqs_hz=[0.1], fs=1.0, decim=65),
               dict(freqs_hz=[0.1], fs=1.0, decim=4, taps=np.zeros(257)), dict(freqs_hz=[0.1], fs=1.0, decim=4, taps=257),
               dict(freqs_hz=[0.1], fs=1.0, decim=4, taps=np.r_[h, np.nan]), dict(freqs_hz=[np.inf], fs=1.0, decim=4),
               dict(freqs_hz=[0.51], fs=1.0, decim=4), dict(freqs_hz=[-1.3e6], fs=2.4e6, decim=4),
               dict(freqs_hz=[0.1], fs=1.0, decim=4, iq_dtype=np.int16)):
        with pytest.raises(ValueError):
            C(**kw)
    lib = sdr.load_library()
    dp = ctypes.POINTER(ctypes.c_double)
    out = ctypes.c_void_p()

    def create(nch, freq, b, decim, dtype=0, taps=None):
        f, t = np.asarray(freq, dtype=np.float64), np.asarray(b, dtype=np.float64)
        return lib.sdr_ddc_create(None, nch, f.ctypes.data_as(dp), t.ctypes.data_as(dp), len(t) if taps is None else taps,
                                  decim, dtype, ctypes.byref(out))
    for args, word in (((0, [0.1], h, 4), "nch"), ((65, np.zeros(65), h, 4), "nch"), ((1, [0.1], h, 0), "decim"),
                       ((1, [0.1], h, 65), "decim"), ((1, [0.1], h, 4, 0, 0), "taps"), ((1, [0.1], h, 4, 0, 257), "taps"),
                       ((1, [0.1], np.r_[h, np.inf], 4), "finite"), ((1, [np.nan], h, 4), "freq"),
                       ((1, [0.50001], h, 4), "freq"), ((1, [0.1], h, 4, 2), "dtype"), ((1, [0.1], h, 4), "context is NULL")):
        assert create(*args) == -1 and word in lib.sdr_last_error().decode(), (args, lib.sdr_last_error())
    assert lib.sdr_ddc_process_dev(None, None, 8, None, 8) == -1
    assert lib.sdr_ddc_run(None, None, 8, None, 8) == -1
    assert lib.sdr_ddc_reset(None, 0) == -1 and lib.sdr_ddc_freq(None, None) == -1 and lib.sdr_ddc_position(None, None) == -1


def split(v):
    v = v.astype(np.float32)
    hi = v.astype(np.float16).astype(np.float32)
    lo = ((v - hi) * LO).astype(np.float16).astype(np.float32)
    return hi, lo


def emulate(xf, nus, h, D, u8=False, inc_of=phase_inc):
    """The kernel's arithmetic in numpy: A (2 rows per channel, K = 2T padded to 32 KS) and the
    window columns split into f16 hi / lo, each 32-wide K step's products summed (f64, rounded
    once: the MFMA's internal order is not modelled) and added to an f32 accumulator, the cross
    terms in a second one, y = acc_c / 2048 + acc_h, then the rotation by the signed 32-bit
    phase rounded to f32 turns, f32 sin / cos and an f32 complex multiply."""
    T = len(h)
    KS = (2 * T + 31) // 32
    K = 32 * KS
    n = len(xf) // 2
    M = n // D
    xp = np.concatenate([np.zeros(2 * (T - 1), np.float32), xf.astype(np.float32), np.zeros(K, np.float32)])
    cols = np.stack([xp[2 * D * m:2 * D * m + K] for m in range(M)], axis=1)          # [K][M]
    bh, bl = split(cols)
    if u8:
        assert not bl.any()
    out = np.empty((len(nus), M), np.complex64)
    m_abs = np.arange(M, dtype=np.uint64) * np.uint64(D)
    for c, nu in enumerate(nus):
        inc = inc_of(nu)
        j = np.arange(T, dtype=np.uint64)
        g = h * np.exp(2j * np.pi * phase_turns(inc, j))
        A = np.zeros((2, K))
        kk = 2 * (T - 1 - np.arange(T))
        A[0, kk], A[0, kk + 1], A[1, kk], A[1, kk + 1] = g.real, -g.imag, g.imag, g.real
        ah, al = split(A.astype(np.float32))
        acc_h = np.zeros((2, M), np.float32)
        acc_c = np.zeros((2, M), np.float32)
        for st in range(KS):
            s = slice(32 * st, 32 * st + 32)
            f = lambda a, b_: a[:, s].astype(np.float64) @ b_[s].astype(np.float64)
            acc_h = (acc_h + f(ah, bh).astype(np.float32)).astype(np.float32)
            acc_c = (acc_c + f(ah, bl).astype(np.float32)).astype(np.float32)
            acc_c = (acc_c + f(al, bh).astype(np.float32)).astype(np.float32)
        y = (acc_c.astype(np.float64) / 2048.0 + acc_h).astype(np.float32)              # one fma
        ph = ((np.uint64(inc) * m_abs) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
        ht = ph.astype(np.float32) * np.float32(2.0 ** -31)
        sn = np.sin(np.pi * ht.astype(np.float64)).astype(np.float32)
        cs = np.cos(np.pi * ht.astype(np.float64)).astype(np.float32)
        re = ((y[0] * cs).astype(np.float32).astype(np.float64) + y[1].astype(np.float64) * sn).astype(np.float32)
        im = ((y[1] * cs).astype(np.float32).astype(np.float64) - y[0].astype(np.float64) * sn).astype(np.float32)
        out[c] = re + 1j * im
    return out


EMU_NUS = (0.0, 0.123456, -0.31, 0.4999, 1 / 3)


@pytest.mark.parametrize("T,D", [(1, 1), (33, 4), (64, 8), (128, 8), (256, 16)])
@pytest.mark.parametrize("kind", ["noise", "tones"])
def test_arithmetic_emulation(sdr, T, D, kind):
    inc_of = sdr.design.ddc_phase_inc                 # the product's quantisation feeds the emulation
    M = 400
    n = M * D
    if kind == "noise":
        xf = noise_iq(n, 11)
    else:
        k = np.arange(n)
        z = sum(a * np.exp(2j * np.pi * (nu * k + 0.1 * i)) for i, (a, nu) in enumerate(zip((1.0, 0.3, 0.5), (0.123456, -0.31, 1 / 3))))
        xf = np.ascontiguousarray(np.stack([z.real, z.imag], axis=1).reshape(-1), dtype=np.float32)
    h = lowpass(T, D)
    x = to_complex(xf)
    ref = ref_ddc(x, EMU_NUS, h, D)
    e = check(emulate(xf, EMU_NUS, h, D, inc_of=inc_of), ref, scale_g(h, x), f"emulation {kind} T={T} D={D}")
    assert e < 5e-7
    if kind == "noise" and T == 64:
        u = noise_iq(n, 12, u8=True)
        xu = to_complex(u, True)
        uf = ((u.astype(np.float32) - 128) / 128).astype(np.float32)
        check(emulate(uf, EMU_NUS, h, D, u8=True, inc_of=inc_of), ref_ddc(xu, EMU_NUS, h, D), scale_g(h, xu), "emulation u8")


def test_emulation_sees_a_dropped_cross_term_and_a_16_bit_phase(sdr):
    """the bound is tight enough to catch the defects it is meant for"""
    T, D, n = 64, 8, 8 * 300
    xf = noise_iq(n, 3)
    h = lowpass(T, D)
    x = to_complex(xf)
    G = scale_g(h, x)
    ref = ref_ddc(x, (0.123456,), h, D)
    inc_of = sdr.design.ddc_phase_inc
    y = emulate(xf, (0.123456,), h, D, inc_of=inc_of)
    assert np.max(np.abs(y - ref)) < 5e-7 * G
    hi = xf.astype(np.float16).astype(np.float32)                     # the x_lo cross term dropped
    assert np.max(np.abs(emulate(hi, (0.123456,), h, D, inc_of=inc_of) - ref)) > 20 * 5e-7 * G
    k = np.arange(len(x) // D, dtype=np.uint64) * np.uint64(D)
    ph16 = np.floor(phase_turns(phase_inc(0.123456), k) * 65536) / 65536     # a 16-bit phase
    y16 = lfilter(h * np.exp(2j * np.pi * phase_turns(phase_inc(0.123456), np.arange(T, dtype=np.uint64))), 1.0, x)[::D] * np.exp(-2j * np.pi * ph16)
    assert np.max(np.abs(y16 - ref)) > 20 * 5e-7 * G


# ---- GPU ------------------------------------------------------------------------------------
def run(sdr, nus, h, D, iq, calls=None, dtype=np.float32, pos=None):
    ch = sdr.Channelizer(np.asarray(nus, dtype=np.float64), 1.0, D, taps=h, iq_dtype=dtype)
    try:
        if pos is not None:
            ch.reset(pos)
        calls = calls or [len(iq) // 2]
        assert sum(calls) == len(iq) // 2
        out, at = [], 0
        for n in calls:
            out.append(ch.process(iq[2 * at:2 * (at + n)]))
            at += n
        return np.concatenate(out, axis=1)
    finally:
        ch.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k0", [0, 1, 3, 4, 32, 33])     # 0, 1, D - 1, D, T - 1, T
def test_impulse(sdr, gpu_ctx, k0):
    T, D, n = 33, 4, 4 * 24
    nus = (0.0, 0.123456, -0.31)
    h = firwin(T, 0.25)
    x = np.zeros(n, np.complex128)
    x[k0] = 1 + 0.5j
    iq = np.ascontiguousarray(np.stack([x.real, x.imag], axis=1).reshape(-1), dtype=np.float32)
    y = run(sdr, nus, h, D, iq)
    # the rotated, decimated taps: y_c[m] = h[mD - k0] (1 + 0.5i) exp(-2 pi i phi_c(k0))
    for c, nu in enumerate(nus):
        m = np.arange(n // D)
        j = m * D - k0
        taps = np.where((j >= 0) & (j < T), h[np.clip(j, 0, T - 1)], 0.0)
        exp = taps * (1 + 0.5j) * np.exp(-2j * np.pi * phase_turns(phase_inc(nu), np.array([k0]))[0])
        assert np.max(np.abs(y[c] - exp)) <= 5e-7 * np.sum(np.abs(h)) * abs(1 + 0.5j), (c, k0)
    check(y, ref_ddc(x, nus, h, D), scale_g(h, x), f"impulse k0={k0}")


MID = dict(nch=9, TD=(64, 8), count=WINDOW + 1)
SHAPES = ([dict(MID, nch=v) for v in (1, 3, 8, 9, 16, 17)] +
          [dict(MID, TD=v) for v in ((1, 1), (15, 1), (16, 4), (17, 4), (65, 8), (128, 10), (256, 64))] +
          [dict(MID, count=v) for v in (1, 15, 16, 17, WINDOW - 1, WINDOW, 3 * WINDOW + 5)] +
          [dict(nch=17, TD=(256, 64), count=3 * WINDOW + 5), dict(nch=16, TD=(64, 8), count=3 * WINDOW + 5)] +
          # the largest 64-output window the staging memory takes (decim 29 at 64 taps), and the first 16-output one
          [dict(nch=3, TD=(64, 29), count=WINDOW + 1), dict(nch=3, TD=(64, 30), count=WINDOW + 1)])


@pytest.mark.gpu
@pytest.mark.parametrize("s", SHAPES, ids=lambda s: f"c{s['nch']}-T{s['TD'][0]}-D{s['TD'][1]}-m{s['count']}")
def test_shapes(sdr, gpu_ctx, s):
    (T, D), nch, M = s["TD"], s["nch"], s["count"]
    h = lowpass(T, D)
    iq = noise_iq(M * D, 100 + T + nch + M)
    nus = nus_for(nch)
    x = to_complex(iq)
    check(run(sdr, nus, h, D, iq), ref_ddc(x, nus, h, D), scale_g(h, x), str(s))


@pytest.mark.gpu
@pytest.mark.parametrize("pos", [0, (1 << 31) + 8 * 12345])
def test_frequencies(sdr, gpu_ctx, pos):
    T, D, M = 64, 8, 2 * WINDOW + 9
    nus = [0.0, 2.0 ** -32, -2.0 ** -32, 0.25, 0.4999, -0.5, 1 / 3, 0.25]
    h = lowpass(T, D)
    iq = noise_iq(M * D, 21)
    x = to_complex(iq)
    y = run(sdr, nus, h, D, iq, pos=pos)
    check(y, ref_ddc(x, nus, h, D, pos), scale_g(h, x), f"frequencies pos={pos}")
    assert np.array_equal(y[3].view(np.uint32), y[7].view(np.uint32))          # the same nu: the same bits
    # rows of the GEMM are independent: channel 11 of 16 is the 1-channel object's row
    many = list(nus_for(16, 5))
    many[11] = 0.123456
    a = run(sdr, [0.123456], h, D, iq, pos=pos)
    b = run(sdr, many, h, D, iq, pos=pos)
    assert np.array_equal(a[0].view(np.uint32), b[11].view(np.uint32))


@pytest.mark.gpu
def test_tones(sdr, gpu_ctx):
    T, D, M = 64, 8, 4 * WINDOW + 3
    nus = (0.123456, -0.31, 1 / 3)
    k = np.arange(M * D)
    z = sum(a * np.exp(2j * np.pi * (phase_inc(nu) / 2.0 ** 32 * k + 0.1 * i)) for i, (a, nu) in enumerate(zip((1.0, 0.3, 0.5), nus)))
    iq = np.ascontiguousarray(np.stack([z.real, z.imag], axis=1).reshape(-1), dtype=np.float32)
    h = lowpass(T, D)
    x = to_complex(iq)
    y = run(sdr, nus, h, D, iq)
    check(y, ref_ddc(x, nus, h, D), scale_g(h, x), "tones")
    # each row settles on its own tone at DC: amplitude a, the others rejected by the low-pass
    for c, a in enumerate((1.0, 0.3, 0.5)):
        assert abs(np.abs(np.mean(y[c, 2 * T // D:])) - a) < 0.02


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
    T, D = 64, 8
    n = 40 * D * 16
    nus = nus_for(3, 9)
    h = lowpass(T, D)
    dt = np.uint8 if u8 else np.float32
    iq = noise_iq(n, 31, u8)
    x = to_complex(iq, u8)
    ref, G = ref_ddc(x, nus, h, D), scale_g(h, x)
    cases = {"one": [n], "by7D": [7 * D] * (n // (7 * D)) + ([n % (7 * D)] if n % (7 * D) else [])}
    if not u8:                                     # (u8: one seam case, the issue's case 7)
        cases.update(byD=[D] * (n // D), uneven=splits(n, D, 4))
    ys = {k: run(sdr, nus, h, D, iq, calls=v, dtype=dt) for k, v in cases.items()}
    for k, y in ys.items():
        check(y, ref, G, f"carried {k} u8={u8}")
        # the splits agree within twice the tolerance (tile alignment moves the accumulation order)
        assert np.all(np.abs(y - ys["one"]) <= 2 * (1e-6 * np.abs(ref) + 5e-7 * G)), k
    ch = sdr.Channelizer(nus, 1.0, D, taps=h, iq_dtype=dt)
    first = ch.process(iq[:2 * 24 * D])
    ch.process(iq[2 * 24 * D:])
    assert ch.position == n
    ch.reset(0)
    assert ch.position == 0
    again = ch.process(iq[:2 * 24 * D])
    assert np.array_equal(first.view(np.uint32), again.view(np.uint32))
    ch.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pos", [(1 << 32) - 8 * 8, 1 << 40])
def test_position(sdr, gpu_ctx, pos):
    T, D = 64, 8
    n = 32 * D
    nus = (0.123456, -0.31, 1 / 3, 0.4999)
    h = lowpass(T, D)
    iq = noise_iq(n, 41)
    x = to_complex(iq)
    ch = sdr.Channelizer(nus, 1.0, D, taps=h)
    ch.reset(pos)
    y = np.concatenate([ch.process(iq[:n]), ch.process(iq[n:])], axis=1)       # two calls of 16 D
    assert ch.position == pos + n
    ch.close()
    check(y, ref_ddc(x, nus, h, D, pos), scale_g(h, x), f"position {pos}")


@pytest.mark.gpu
def test_u8_middle_setting(sdr, gpu_ctx):
    (T, D), nch, M = MID["TD"], MID["nch"], MID["count"]
    h = lowpass(T, D)
    iq = noise_iq(M * D, 51, u8=True)
    x = to_complex(iq, True)
    nus = nus_for(nch)
    check(run(sdr, nus, h, D, iq, dtype=np.uint8), ref_ddc(x, nus, h, D), scale_g(h, x), "u8 middle")
    # an odd split puts the second call's first byte at every 4-byte phase of the staging loads
    y = run(sdr, nus, h, D, iq, calls=[D, 3 * D, (M - 4) * D], dtype=np.uint8)
    check(y, ref_ddc(x, nus, h, D), scale_g(h, x), "u8 split")


@pytest.mark.gpu
@pytest.mark.parametrize("T", [64, 65])
@pytest.mark.parametrize("shift", [0, 2])
def test_u8_byte_alignment(sdr, gpu_ctx, T, shift):
    """u8 windows start at any even byte: the staging loads are 4-byte words, so a window that
    starts 2 bytes past a word boundary is staged from the word before.  T = 64 / 65 and a
    device pointer 0 / 2 bytes past an aligned one give both phases with and without history."""
    D, M, nch = 8, 2 * WINDOW + 3, 3
    n = M * D
    h = lowpass(T, D)
    nus = nus_for(nch, 13)
    iq = noise_iq(n, 71, u8=True)
    x = to_complex(iq, True)
    buf = sdr.DeviceBuffer(gpu_ctx, 2 * n + 16)
    buf.upload(iq, offset=shift)
    out = sdr.DeviceBuffer(gpu_ctx, nch * M * 8)
    ch = sdr.Channelizer(nus, 1.0, D, taps=h, iq_dtype=np.uint8, ctx=gpu_ctx)
    half = (M // 2) * D                                 # two calls: the second starts inside the buffer
    ch.process_dev(buf.ptr + shift, half, out.ptr, M)
    ch.process_dev(buf.ptr + shift + 2 * half, n - half, out.ptr + 8 * (M // 2), M)
    gpu_ctx.synchronize()
    y = out.download(nch * M * 2, np.float32).view(np.complex64).reshape(nch, M)
    check(y, ref_ddc(x, nus, h, D), scale_g(h, x), f"u8 alignment T={T} shift={shift}")
    with pytest.raises(ValueError):
        ch.process_dev(buf.ptr + 1, n, out.ptr, M)      # an odd address: not a whole complex sample
    ch.close()
    buf.free()
    out.free()


@pytest.mark.gpu
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_run_equals_process_dev_and_strides(sdr, gpu_ctx, u8):
    T, D, M, nch = 64, 8, 2 * WINDOW + 7, 5
    n, stride = M * D, M + 9
    h = lowpass(T, D)
    nus = nus_for(nch, 3)
    iq = noise_iq(n, 61, u8)
    lib = gpu_ctx.lib
    ch = sdr.Channelizer(nus, 1.0, D, taps=h, iq_dtype=np.uint8 if u8 else np.float32, ctx=gpu_ctx)
    packed = ch.process(iq)
    # the host path with a row stride: gaps untouched
    host = np.full((nch, stride), np.complex64(7 - 3j))
    ch.reset(0)
    assert lib.sdr_ddc_run(ch.handle, iq.ctypes.data, n, host.ctypes.data, stride) == 0
    assert np.array_equal(host[:, :M].view(np.uint32), packed.view(np.uint32))
    assert np.all(host[:, M:] == np.complex64(7 - 3j))
    # the device path, poison in the gaps
    poison = np.full(nch * stride * 2 + 16, 0xABABABAB, np.uint32)
    din = sdr.DeviceBuffer.from_array(gpu_ctx, iq)
    dout = sdr.DeviceBuffer.from_array(gpu_ctx, poison)
    ch.reset(0)
    ch.process_dev(din.ptr, n, dout.ptr, stride)
    gpu_ctx.synchronize()
    got = dout.download(len(poison), np.uint32)
    rows = got[:nch * stride * 2].reshape(nch, 2 * stride)
    assert np.array_equal(rows[:, :2 * M], packed.view(np.uint32))
    assert np.all(rows[:, 2 * M:] == 0xABABABAB) and np.all(got[nch * stride * 2:] == 0xABABABAB)
    assert ch.position == n
    # call-time argument errors: refused before any launch, the position unchanged
    for args in ((din.ptr, n - 1, dout.ptr, stride), (din.ptr, 0, dout.ptr, stride), (din.ptr, n, dout.ptr, M - 1)):
        with pytest.raises(ValueError):
            ch.process_dev(*args)
        assert lib.sdr_ddc_process_dev(ch.handle, *args) == -1
    with pytest.raises(ValueError):
        ch.process(iq[:2 * (D + 1)])
    for bad in (-8, 3):
        with pytest.raises(ValueError):
            ch.reset(bad)
    assert ch.position == n
    assert np.allclose(ch.freqs_hz, [sdr.design.ddc_actual_freq(phase_inc(v)) for v in nus], rtol=0, atol=0)
    din.free()
    dout.free()
    ch.close()


@pytest.mark.gpu
def test_into_the_receiver(sdr, gpu_ctx):
    """capture -> channelizer -> receiver without leaving HBM, against the f64 reference
    channelizer's rows (rounded to f32) through an identically configured receiver.
    Bound 2e-5 on the audio: a relative IQ error eps moves the arctan demod by <= 2 eps rad,
    the audio filter's sum|b| is below 3, and eps <= 1.5e-6 G / amplitude here."""
    B, UP, nst = 51200, 8, 3
    nus = (-0.25, 0.0371, 0.3)
    n_nb = 2 * B
    n = n_nb * UP
    k = np.arange(n)
    wide = np.zeros(n, np.complex128)
    for s, (nu, snr) in enumerate(zip(nus, (30.0, 20.0, 25.0))):
        st = sdr.synth.fm_iq(n_nb, seed=s + 1, snr_db=snr).astype(np.float64)
        z = resample_poly(st[0::2] + 1j * st[1::2], UP, 1)                # zero-stuff x8 and low-pass
        wide += z * np.exp(2j * np.pi * (phase_inc(nu) / 2.0 ** 32) * k)
    wide *= 0.3
    iq = np.ascontiguousarray(np.stack([wide.real, wide.imag], axis=1).reshape(-1), dtype=np.float32)
    h = sdr.design.channel_coeffs(UP)
    assert len(h) == 64
    stride = (n_nb + 31) // 32 * 32
    ch = sdr.Channelizer(nus, 1.0, UP, taps=h, ctx=gpu_ctx)
    din = sdr.DeviceBuffer.from_array(gpu_ctx, iq)
    rows = sdr.DeviceBuffer(gpu_ctx, nst * stride * 8)
    ch.process_dev(din.ptr, n, rows.ptr, stride)
    ref = ref_ddc(to_complex(iq), nus, h, UP).astype(np.complex64)
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
    print(f"ddc into the receiver: audio max |a - b| = {err:.3e} (audio peak {np.max(np.abs(b)):.3f})")
    assert a.shape == (nst, 2 * (B // 10 // 5)) and np.all(np.isfinite(a))
    assert err <= 2e-5, err
    for i in range(nst):
        for j in range(i + 1, nst):
            assert np.max(np.abs(a[i] - a[j])) > 1e-2, (i, j)           # no swapped or repeated row
    for d in (din, rows, dref):
        d.free()
    ch.close()
