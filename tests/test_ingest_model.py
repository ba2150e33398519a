"""The capture ingest rule (rtsdr.ingest_model, capture.py) pinned independently of its
implementation: the conversion of every code of every integer format, the pass-through of float32,
the level meter against plain Python-integer loops, the format names, and the argument errors of
rtsdr.CaptureIngest raised before a context exists.  No GPU."""
import math
import warnings

import numpy as np
import pytest

INT_FORMATS = (("cu8", np.uint8, 8), ("cs8", np.int8, 8), ("cs16", np.int16, 16))


def exhaustive(dtype):
    """every value of the type: I ascending, Q descending"""
    info = np.iinfo(dtype)
    v = np.arange(info.min, info.max + 1, dtype=np.int64)
    x = np.empty(2 * len(v), dtype=dtype)
    x[0::2] = v.astype(dtype)
    x[1::2] = v[::-1].astype(dtype)
    return x


def codes_of(x, fmt):
    return [int(v) - (128 if fmt == "cu8" else 0) for v in x]


def loop_meter(x, fmt, bits):
    """the integer meter by the letter of the rule, in Python integers"""
    c = codes_of(x, fmt)
    hi, lo = 2 ** (bits - 1) - 1, -2 ** (bits - 1)
    clipped = peak = sumsq = 0
    for ci, cq in zip(c[0::2], c[1::2]):
        clipped += int(ci >= hi or ci <= lo or cq >= hi or cq <= lo)
        peak = max(peak, abs(ci), abs(cq))
        sumsq += ci * ci + cq * cq
    return len(c) // 2, clipped, peak, sumsq


@pytest.mark.parametrize("fmt,dtype,bits", INT_FORMATS)
def test_every_code(sdr, fmt, dtype, bits):
    x = exhaustive(dtype)
    out, m = sdr.ingest_model(x, fmt)
    c = np.array(codes_of(x, fmt), dtype=np.float64)
    want = (c / 2.0 ** (bits - 1)).astype(np.float32)
    assert out.dtype == np.float32 and out.shape == x.shape and np.array_equal(out, want)
    assert np.array_equal(out.astype(np.float64) * 2.0 ** (bits - 1), c)          # the rounding to f32 was exact
    assert np.array_equal(sdr.ingest_model(x, dtype)[0], out)                     # the dtype as a synonym
    n, clipped, peak, sumsq = loop_meter(x, fmt, bits)
    assert (m.n, m.clipped, m.nonfinite, m.peak_code, m.sumsq_code) == (n, clipped, 0, peak, sumsq)
    assert clipped == 2 and peak == 2 ** (bits - 1)                               # the first and the last sample hold both rails
    assert m.peak == 1.0 and m.sumsq == sumsq / 4.0 ** (bits - 1)
    assert (m.calls, m.total_n, m.total_clipped) == (1, n, clipped)
    if fmt == "cu8":
        assert np.array_equal(out, (x.astype(np.float32) - 128.0) / 128.0)        # the project's u8 rule


def test_bits_12(sdr):
    rng = np.random.default_rng(0)
    x = rng.integers(-2048, 2048, 2 * 500).astype(np.int16)
    x[10], x[21], x[40] = 2047, -2048, 2046
    out, m = sdr.ingest_model(x, "cs16", bits=12)
    assert np.array_equal(out, (x.astype(np.float64) / 2048.0).astype(np.float32)) and np.max(np.abs(out)) == 1.0
    n, clipped, peak, sumsq = loop_meter(x, "cs16", 12)
    assert (m.n, m.clipped, m.peak_code, m.sumsq_code) == (n, clipped, peak, sumsq) and peak == 2048
    assert clipped >= 2                                                           # x[10] and x[21]; x[40] is one short of the rail
    assert m.peak == 1.0 and m.sumsq == sumsq / 2048.0 ** 2
    # codes beyond the 12 bits: converted by the same scale, and counted as clipped
    y = np.array([3000, 5, -5, -2049, 100, 100, 32767, -32768], dtype=np.int16)
    out, m = sdr.ingest_model(y, "cs16", bits=12)
    assert list(out) == [3000 / 2048, 5 / 2048, -5 / 2048, -2049 / 2048, 100 / 2048, 100 / 2048, 32767 / 2048, -16.0]
    assert (m.clipped, m.peak_code, m.sumsq_code) == (3, 32768, sum(int(v) ** 2 for v in y))
    assert m.peak == 16.0
    for bits in (2, 7, 16):
        out, m = sdr.ingest_model(y, "cs16", bits=bits)
        assert np.array_equal(out, (y / 2.0 ** (bits - 1)).astype(np.float32)) and m.sumsq_code == sum(int(v) ** 2 for v in y)


@pytest.mark.parametrize("fmt,dtype,bits", INT_FORMATS)
def test_each_rail(sdr, fmt, dtype, bits):
    hi, lo = 2 ** (bits - 1) - 1, -2 ** (bits - 1)
    off = 128 if fmt == "cu8" else 0
    quiet = [3, -4, 0, 1, hi - 1, lo + 1]                      # one short of each rail: not clipped
    assert sdr.ingest_model((np.array(quiet, np.int64) + off).astype(dtype), fmt)[1].clipped == 0
    for k in range(4):                                          # the high rail on I, on Q; the low rail on I, on Q
        codes = list(quiet)
        codes[2 + k % 2] = hi if k < 2 else lo
        m = sdr.ingest_model((np.array(codes, np.int64) + off).astype(dtype), fmt)[1]
        assert (m.clipped, m.peak_code) == (1, hi if k < 2 else -lo), k
    both = (np.array([hi, lo, lo, lo, hi, hi], np.int64) + off).astype(dtype)   # a sample counts once
    assert sdr.ingest_model(both, fmt)[1].clipped == 3


def test_swap(sdr):
    x = np.array([1, 2, 3, 4, -128, 127], dtype=np.int8)
    a, ma = sdr.ingest_model(x, "cs8")
    b, mb = sdr.ingest_model(x, "cs8", swap=True)
    assert np.array_equal(b[0::2], a[1::2]) and np.array_equal(b[1::2], a[0::2]) and ma == mb
    f = np.array([0.5, np.nan, -2.0, 0.25], dtype=np.float32)
    b, mb = sdr.ingest_model(f, "cf32", swap=True)
    assert np.array_equal(b.view(np.uint32), f[[1, 0, 3, 2]].view(np.uint32)) and mb == sdr.ingest_model(f, "cf32")[1]


def test_cf32_passes_through(sdr):
    rng = np.random.default_rng(1)
    x = rng.standard_normal(2 * 300).astype(np.float32) * np.float32(0.4)
    x[7], x[20], x[21], x[100] = np.nan, np.inf, 0.5, -np.inf
    x[50] = -1.0                                                 # clipped, and the peak of the finite samples
    bits = x.view(np.uint32).copy()
    bits[301] = 0x7fc12345                                       # a NaN with a payload
    x = bits.view(np.float32)
    out, m = sdr.ingest_model(x, np.float32)
    assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), bits) and out is not x
    fin = [(float(a), float(b)) for a, b in zip(x[0::2], x[1::2]) if math.isfinite(a) and math.isfinite(b)]
    assert m.n == 300 and m.nonfinite == 300 - len(fin) == 4 and (m.peak_code, m.sumsq_code) == (0, 0)
    assert m.clipped == sum(1 for a, b in fin if abs(a) >= 1 or abs(b) >= 1) and m.clipped >= 1
    assert m.peak == max(max(abs(a), abs(b)) for a, b in fin)
    want = math.fsum(a * a + b * b for a, b in fin)
    assert abs(m.sumsq - want) <= 300 * 2.0 ** -52 * want
    assert sdr.ingest_model(x.view(np.complex64), "cf32")[0].tobytes() == x.tobytes()
    assert sdr.ingest_model(x.view(np.uint8), "cf32")[1] == m                    # raw bytes


def test_carried_totals(sdr):
    a = np.array([127, 0, 1, 1], np.int8)
    b = np.array([5, 5, -128, 3, 127, 127], np.int8)
    _, m1 = sdr.ingest_model(a, "cs8")
    _, m2 = sdr.ingest_model(b, "cs8", prev=m1)
    _, m3 = sdr.ingest_model(a, "cs8", prev=m2)
    assert (m2.n, m2.clipped, m2.calls, m2.total_n, m2.total_clipped) == (3, 2, 2, 5, 3)
    assert (m3.n, m3.clipped, m3.calls, m3.total_n, m3.total_clipped) == (2, 1, 3, 7, 4)
    assert sdr.ingest_model(a, "cs8", prev=None)[1] == m1


def test_dbfs_helpers(sdr):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for fmt, x in (("cs16", np.zeros(64, np.int16)), ("cu8", np.full(64, 128, np.uint8)), ("cf32", np.zeros(64, np.float32))):
            m = sdr.ingest_model(x, fmt)[1]
            assert m.power_dbfs == -math.inf and m.peak_dbfs == -math.inf and m.clip_share == 0.0
        m = sdr.ingest_model(np.full(8, np.nan, np.float32), "cf32")[1]           # no finite sample at all
        assert m.nonfinite == 4 and m.power_dbfs == -math.inf and m.peak_dbfs == -math.inf
    # a full-scale square wave on I and Q is 0 dBFS; half scale is 20 log10(1/2)
    m = sdr.ingest_model(np.full(32, -128, np.int8), "cs8")[1]
    assert m.power_dbfs == 0.0 and m.peak_dbfs == 0.0 and m.clip_share == 1.0
    m = sdr.ingest_model(np.tile(np.array([1024, -1024], np.int16), 8), "cs16", bits=12)[1]
    assert math.isclose(m.power_dbfs, 20 * math.log10(0.5), abs_tol=1e-12) and math.isclose(m.peak_dbfs, 20 * math.log10(0.5), abs_tol=1e-12)
    m = sdr.ingest_model(np.array([0.5, np.nan, 0.25, 0.25], np.float32), "cf32")[1]   # the NaN sample is left out of the mean
    assert math.isclose(m.power_dbfs, 10 * math.log10(0.0625), abs_tol=1e-12)


def test_capture_format(sdr):
    f = sdr.capture_format
    for name, want in (("band.cs8", "cs8"), ("/data/run.1/fm_20M.CS16", "cs16"), ("x.cu8", "cu8"), ("a.b.Cf32", "cf32"),
                       ("cu8", "cu8"), ("ci8", "cs8"), ("ci16_le", "cs16"), ("cf32_le", "cf32"), ("cs8", "cs8"), ("cs16", "cs16"),
                       ("cf32", "cf32"), ("CI16_LE", "cs16")):
        assert f(name) == want, name
    for bad in ("band.wav", "ci16_be", "cf64_le", "ri16_le", "", "band.cs12", "cs8.bin", None, 8, np.int8):
        with pytest.raises(ValueError):
            f(bad)


def test_model_refusals(sdr):
    x8, x16 = np.zeros(8, np.int8), np.zeros(8, np.int16)
    for args in ((x8, "cs12"), (x8, np.int32), (x8, "cs8", 7), (x8, "cs8", 16), (x8.view(np.uint8), "cu8", 12), (x16, "cs16", 1), (x16, "cs16", 17),
                 (x16, "cs16", 12.5), (np.zeros(8, np.float32), "cf32", 16), (x16, "cs8"), (x8[:7], "cs8"), (x8[:0], "cs8"),
                 (x8.reshape(2, 4), "cs8"), (np.zeros(6, np.uint8), "cs16")):
        with pytest.raises(ValueError):
            sdr.ingest_model(*args)
    assert sdr.ingest_model(x8, "cs8", 8)[1].n == 4 and sdr.ingest_model(np.zeros(8, np.float32), "cf32", 32)[1].n == 4


def test_capture_ingest_argument_errors_before_a_context(sdr):
    """nothing here loads the library or opens a device: the objects are never opened"""
    C = sdr.CaptureIngest
    for kw in (dict(fmt="cs12"), dict(fmt=np.int32), dict(fmt="cs8", bits=12), dict(fmt="cu8", bits=7), dict(fmt="cs16", bits=1),
               dict(fmt="cs16", bits=17), dict(fmt="cf32", bits=16), dict(fmt=None)):
        with pytest.raises(ValueError):
            C(**kw)
    c8, c16, cf = C("cs8"), C(np.int16, bits=12, swap=True), C("cf32", meter=False)
    assert (c8.fmt, c8.bits, c8.es) == ("cs8", 8, 2) and (c16.fmt, c16.bits, c16.es, c16.swap) == ("cs16", 12, 4, True)
    assert (cf.fmt, cf.bits, cf.es, cf.metered) == ("cf32", 32, 8, False) and C.CHUNK == 4096
    for c, args in ((c8, (0, 8, 4096)), (c8, (4096, 8, 0)), (c8, (4096, 0, 65536)), (c8, (4096, 2 ** 31, 1 << 40)),
                    (c8, (4097, 8, 65536)), (c16, (4098, 8, 65536)), (cf, (4100, 8, 65536)), (c8, (4096, 8, 65540)),
                    (c8, (4096, 8, 4096)), (c16, (4096 + 28, 8, 4096)), (c8, (4100, 8, 4096 - 56)), (cf, (4096, 8, 4104)), (cf, (4104, 8, 4096))):
        with pytest.raises(ValueError):
            c.process_dev(*args)
    for c, raw in ((c8, np.zeros(7, np.int8)), (c8, np.zeros(8, np.int16)), (c16, np.zeros(0, np.int16)), (cf, np.zeros(8, np.float64))):
        with pytest.raises(ValueError):
            c.run(raw)
    assert all(c.handle is None for c in (c8, c16, cf))
