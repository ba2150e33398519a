"""The IQ-correction rule on the CPU: rtsdr.IqBalance (iqbalance.py, numpy f64), the specification of
the device stage (tests/test_iqc.py), on the synthetic capture of tests/iqc_capture.py; and the
argument checks of rtsdr.IqCorrector and of the C entry points, none of which needs a GPU.

The bounds on the capture are the issue's: the image of the two strongest stations improves by at
least 20 dB in one block, c1 and c2 are within 2e-3 of -tan 4deg and 1 / (1.06 cos 4deg), the output's
mean is below 1e-6, and an unimpaired capture keeps its images at -50 dB or below."""
import ctypes
import math

import numpy as np
import pytest

import iqc_capture as cap

DTYPES = (np.float32, np.uint8)
STRONGEST = (3.1e6, -5.3e6)


def _pairs(iq):
    x = np.asarray(iq).astype(np.float64)
    if np.asarray(iq).dtype == np.uint8:
        x = (x - 128.0) / 128.0
    return x[0::2], x[1::2]


def _moments(iq):
    i, q = _pairs(iq)
    n = len(i)
    return np.array([math.fsum(i) / n, math.fsum(q) / n, math.fsum(i * i) / n, math.fsum(q * q) / n, math.fsum(i * q) / n])


@pytest.mark.parametrize("n", (8192, 32771))
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_block_removes_image_and_dc(sdr, dtype, n):
    x = cap.capture(n, dtype)
    m = sdr.IqBalance(dtype)
    y = m.process(x)
    st = m.state()
    assert y.dtype == np.float32 and y.shape == (2 * n,)
    for f in STRONGEST:
        before, after = cap.image_db(x, f), cap.image_db(y, f)
        print(f"{np.dtype(dtype).name} n={n} f={f / 1e6:+.1f} MHz: image {before:.1f} -> {after:.1f} dB")
        assert before - after >= 20.0
    print(f"c1 - (-tan 4deg) = {st.c1 - cap.C1:.2e}, c2 - 1/(1.06 cos 4deg) = {st.c2 - cap.C2:.2e}, image_db {st.image_db:.1f}")
    assert abs(st.c1 - cap.C1) <= 2e-3 and abs(st.c2 - cap.C2) <= 2e-3
    assert abs(np.mean(y[0::2], dtype=np.float64)) < 1e-6 and abs(np.mean(y[1::2], dtype=np.float64)) < 1e-6
    assert (st.updates, st.skipped, st.holds) == (1, 0, 0)
    assert (st.dI, st.dQ) == (st.mI, st.mQ)
    # a quarter of the impropriety is the image ratio of a small imbalance: about -27 dB here
    assert abs(st.image_db - cap.image_db(x, 3.1e6)) < 1.0 and st.impropriety == m.impropriety


@pytest.mark.parametrize("n", (8192, 32771))
@pytest.mark.parametrize("dtype", DTYPES)
def test_unimpaired_capture_stays_unimpaired(sdr, dtype, n):
    x = cap.capture(n, dtype, impaired=False)
    m = sdr.IqBalance(dtype)
    y = m.process(x)
    for f in STRONGEST:
        print(f"{np.dtype(dtype).name} n={n} f={f / 1e6:+.1f} MHz: image {cap.image_db(x, f):.1f} -> {cap.image_db(y, f):.1f} dB")
        assert cap.image_db(y, f) <= -50.0
    assert abs(m.state().c1) < 2e-3 and abs(m.state().c2 - 1.0) < 2e-3


@pytest.mark.parametrize("dtype", DTYPES)
def test_smoothing_over_four_blocks(sdr, dtype):
    """m = r on the first update, m + rate (r - m) later, by hand on fsum moments (the f32 sums are
    numpy's pairwise ones: equal to fsum's to a few ulps, hence the 1e-13)."""
    lens = (1000, 777, 2048, 1)
    x = cap.capture(sum(lens), dtype)
    m = sdr.IqBalance(dtype, rate=0.25)
    want, o = None, 0
    for k, n in enumerate(lens):
        blk = x[2 * o:2 * (o + n)]
        o += n
        y = m.process(blk)
        r = _moments(blk)
        want = r if k == 0 else want + 0.25 * (r - want)
        st = m.state()
        got = np.array(st[:5])
        if dtype == np.uint8:
            assert np.array_equal(got, want)                       # exact sums, the same operations
        else:
            assert np.allclose(got, want, rtol=1e-13, atol=0.0)
        assert st.updates == k + 1
        # the coefficients are step 3 of the smoothed moments, and the block is mapped with them
        A, B, C = got[2] - got[0] ** 2, got[3] - got[1] ** 2, got[4] - got[0] * got[1]
        t = B - (C / A) * C
        assert A > 0 and t > 0
        assert st.c2 == math.sqrt(A / t) and st.c1 == -(C / A) * st.c2 and (st.dI, st.dQ) == (got[0], got[1])
        i, q = _pairs(blk)
        ref = np.empty(2 * n, dtype=np.float32)
        ref[0::2] = i - st.dI
        ref[1::2] = st.c1 * (i - st.dI) + st.c2 * (q - st.dQ)
        assert np.array_equal(y, ref)
    # (the one-sample block alone has A = 0; the smoothed moments it enters stay valid)
    assert m.state().holds == 0


def _hold_blocks(dtype):
    n = 300
    if dtype == np.uint8:
        zero = np.full(2 * n, 128, np.uint8)
        const = np.tile(np.array([200, 56], np.uint8), n)             # (0.5625, -0.5625): exact squares
        ramp = np.arange(n, dtype=np.uint8)
    else:
        zero = np.zeros(2 * n, np.float32)
        const = np.tile(np.array([0.25, -0.5], np.float32), n)
        ramp = (np.arange(n) / 256.0 - 0.5).astype(np.float32)
    same = np.repeat(ramp, 2)                                        # Q = I
    return zero, const, same


@pytest.mark.parametrize("dtype", DTYPES)
def test_hold_cases(sdr, dtype):
    m = sdr.IqBalance(dtype)
    m.process(cap.capture(4096, dtype))
    coeff = m.state()[5:9]
    for k, blk in enumerate(_hold_blocks(dtype)):
        m2 = sdr.IqBalance(dtype, rate=1.0)                           # rate 1: the block's own moments
        m2.set(*coeff)
        y = m2.process(blk)
        st = m2.state()
        assert st[5:9] == coeff and (st.updates, st.skipped, st.holds) == (1, 0, 1), k
        i, q = _pairs(blk)
        assert np.array_equal(y[0::2], (i - coeff[0]).astype(np.float32))
    # and from the initial state the identity stays
    m3 = sdr.IqBalance(dtype)
    blk = _hold_blocks(dtype)[0]
    y = m3.process(blk)
    assert m3.state()[5:9] == (0.0, 0.0, 0.0, 1.0) and m3.state().holds == 1 and not np.any(y)


def test_nan_block_is_skipped_and_mapped_with_old_coefficients(sdr):
    m = sdr.IqBalance()
    x = cap.capture(4096)
    m.process(x)
    before = m.state()
    blk = np.array(cap.capture(8192)[2 * 4096:])
    blk[2 * 100] = np.nan                                            # I of sample 100
    blk[2 * 200 + 1] = np.nan                                        # Q of sample 200
    y = m.process(blk)
    st = m.state()
    assert st[:9] == before[:9] and (st.updates, st.skipped, st.holds) == (1, 1, 0)
    ref = sdr.IqBalance()
    ref.set(*before[5:9])
    want = ref.process(blk, estimate=False)
    assert np.array_equal(y, want, equal_nan=True)
    nan = np.flatnonzero(np.isnan(y))
    assert list(nan) == [200, 201, 401]                              # I and Q of sample 100, Q of sample 200
    blk[2 * 100] = np.inf                                            # an infinity: a non-finite moment too
    m.process(blk)
    assert m.state().skipped == 2 and m.state()[:9] == before[:9]


@pytest.mark.parametrize("dtype", DTYPES)
def test_flags_set_and_reset(sdr, dtype):
    x = cap.capture(8192, dtype)
    i, q = _pairs(x)
    full = sdr.IqBalance(dtype)
    full.process(x)
    f = full.state()
    nodc = sdr.IqBalance(dtype, dc=False)
    y = nodc.process(x)
    st = nodc.state()
    assert (st.dI, st.dQ) == (0.0, 0.0) and (st.c1, st.c2) == (f.c1, f.c2)   # the moments are still central
    assert abs(np.mean(y[0::2], dtype=np.float64) - f.mI) < 1e-6
    nobal = sdr.IqBalance(dtype, balance=False)
    y = nobal.process(x)
    st = nobal.state()
    assert (st.c1, st.c2) == (0.0, 1.0) and (st.dI, st.dQ) == (f.dI, f.dQ)
    assert np.array_equal(y[1::2], (q - f.dQ).astype(np.float32))
    # estimate off: the coefficients in force, the state untouched
    m = sdr.IqBalance(dtype)
    y = m.process(x, estimate=False)
    assert m.state().updates == 0 and np.array_equal(y[0::2], i.astype(np.float32)) and np.array_equal(y[1::2], q.astype(np.float32))
    m.set(0.03, -0.02, cap.C1, cap.C2)
    y = m.process(x, estimate=False)
    assert m.state()[5:9] == (0.03, -0.02, cap.C1, cap.C2) and m.state().updates == 0
    assert cap.image_db(x, 3.1e6) - cap.image_db(y, 3.1e6) >= 20.0
    m.process(x)
    assert m.state().updates == 1
    m.reset()
    assert m.state()[:12] == (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0, 0, 0) and math.isnan(m.state().impropriety)
    # complex input for a float32 object
    if dtype == np.float32:
        z = (i + 1j * q).astype(np.complex64)
        assert np.array_equal(sdr.IqBalance().process(z), sdr.IqBalance().process(x))


def test_argument_errors_before_device_work(sdr):
    """Python raises ValueError before a context exists; the C entry points refuse the same
    arguments (SDR_EINVAL with a message) before they look at their context."""
    for cls in (sdr.IqBalance, sdr.IqCorrector):
        for kw in (dict(iq_dtype=np.int16), dict(rate=0.0), dict(rate=-0.1), dict(rate=1.5), dict(rate=np.nan), dict(rate=np.inf)):
            with pytest.raises(ValueError):
                cls(**kw)
    c8, cf = sdr.IqCorrector(np.uint8), sdr.IqCorrector()
    for c, args in ((cf, (0, 8, 4096)), (cf, (4096, 8, 0)), (cf, (4096, 0, 65536)), (cf, (4096, 2 ** 31, 1 << 40)),
                    (cf, (4100, 8, 65536)), (cf, (4096, 8, 65540)), (c8, (4097, 8, 65536)), (c8, (4096, 8, 65540)),
                    (cf, (4096, 8, 4104)), (cf, (4104, 8, 4096)), (c8, (4096, 8, 4096)), (c8, (4100, 8, 4096 - 56))):
        with pytest.raises(ValueError):
            c.process_dev(*args)
    for bad in ((1.0, 2.0, 3.0, np.nan), (np.inf, 0.0, 0.0, 1.0)):
        with pytest.raises(ValueError):
            cf.set(*bad)
        with pytest.raises(ValueError):
            sdr.IqBalance().set(*bad)
    for bad in (np.zeros(3, np.float32), np.zeros(0, np.float32), np.zeros((2, 2), np.float32)):
        with pytest.raises(ValueError):
            cf.run(bad)
        with pytest.raises(ValueError):
            sdr.IqBalance().process(bad)
    with pytest.raises(ValueError):
        c8.run(np.zeros(4, np.complex64))
    assert cf.handle is None and c8.handle is None                   # no context was asked for

    lib = sdr.load_library()
    out = ctypes.c_void_p()

    class Params(ctypes.Structure):
        _fields_ = [("rate", ctypes.c_double), ("dc", ctypes.c_int), ("balance", ctypes.c_int)]

    def create(dtype, rate=None, out_ref=ctypes.byref(out)):
        prm = ctypes.byref(Params(rate, 1, 1)) if rate is not None else None
        return lib.sdr_iqc_create(None, dtype, prm, out_ref)
    for args, word in (((0, None, None), "out is NULL"), ((2,), "dtype"), ((-1,), "dtype"), ((0, 0.0), "rate"), ((1, 1.0001), "rate"),
                       ((0, float("nan")), "rate"), ((0, float("inf")), "rate"), ((0,), "context is NULL"), ((1, 1.0), "context is NULL")):
        assert create(*args) == -1 and word in lib.sdr_last_error().decode(), (args, lib.sdr_last_error())
    assert lib.sdr_iqc_process_dev(None, None, 8, None, 1) == -1 and "NULL" in lib.sdr_last_error().decode()
    assert lib.sdr_iqc_run(None, None, 8, None, 1) == -1 and "NULL" in lib.sdr_last_error().decode()
    assert lib.sdr_iqc_reset(None) == -1 and lib.sdr_iqc_set(None, None) == -1
    assert lib.sdr_iqc_state(None, None) == -1 and lib.sdr_iqc_coeffs_dev(None, None) == -1
    lib.sdr_iqc_destroy(None)
