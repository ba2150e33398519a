"""The device-side capture ingest (CaptureIngest, csrc/ingest.hip) against the host rule
rtsdr.ingest_model (tests/test_ingest_model.py pins that on the CPU), and the C entry points'
refusals.

What is compared, after every call: out bit for bit; the meter's integer fields (n, clipped,
nonfinite, peak_code, sumsq_code) and the carried totals exactly; peak exactly; sumsq exactly for the
integer formats (it is derived from sumsq_code) and, for cf32, within a relative n 2^-52 of numpy's
f64 sum -- the bound of any summation order over non-negative terms, so it does not constrain the
chunking.  The input sits between guards that a stray read would show in the meter (values on a
rail, 1e30 for cf32), the output between guards of a float pattern that must come back untouched."""
import ctypes

import numpy as np
import pytest

gpu = pytest.mark.gpu

CHUNK = 4096         # samples of a workgroup's chunk, at least (include/sdr.h SDR_INGEST_CHUNK, CaptureIngest.CHUNK)
EDGES = (1, 2, 7, 8, 9, 15, 17, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
FORMATS = {"cu8": np.uint8, "cs8": np.int8, "cs16": np.int16, "cf32": np.float32}
GUARD = 64                                     # floats on either side of out
IN_GUARD = 64                                  # bytes on either side of raw
SENTINEL = np.float32(-7.25e12)


def rail(dtype):
    return np.float32(1e30) if dtype == np.float32 else np.iinfo(dtype).max


def random_block(fmt, n, seed=0):
    """random values of the format with both rails present; cf32: a share beyond +-1 and, from 8
    samples on, a NaN, an infinity and a NaN with a payload"""
    dtype = FORMATS[fmt]
    rng = np.random.default_rng([seed, n])
    if fmt == "cf32":
        x = (0.5 * rng.standard_normal(2 * n)).astype(np.float32)
        x[0], x[-1] = 1.0, -1.5
        if n >= 8:
            x[5], x[2 * n - 4] = np.nan, -np.inf
            x.view(np.uint32)[9] = 0xffc00abc
        return x
    info = np.iinfo(dtype)
    x = rng.integers(info.min, info.max + 1, 2 * n).astype(dtype)
    x[0], x[-1] = info.max, info.min
    return x


class Bench:
    """One input and one output allocation, reused by the calls of a test."""

    def __init__(self, sdr, ctx, fmt, nmax):
        self.sdr, self.ctx, self.dtype = sdr, ctx, np.dtype(FORMATS[fmt])
        self.es = 2 * self.dtype.itemsize
        self.bin = sdr.DeviceBuffer(ctx, self.es * (nmax + 8) + 2 * IN_GUARD)
        self.bout = sdr.DeviceBuffer(ctx, 4 * (2 * nmax + 2 * GUARD + 8))
        assert self.bin.ptr % 256 == 0 and self.bout.ptr % 256 == 0

    def place(self, x, in_off):
        """x uploaded in_off samples past a 16-byte boundary, rail values around it -> its pointer"""
        g = IN_GUARD // self.dtype.itemsize
        host = np.full(2 * g + 2 * in_off + len(x), rail(self.dtype.type), dtype=self.dtype)
        host[g + 2 * in_off:g + 2 * in_off + len(x)] = x
        self.bin.upload(host)
        ptr = self.bin.ptr + IN_GUARD + self.es * in_off
        assert (ptr - self.es * in_off) % 16 == 0
        return ptr

    def call(self, ing, x, in_off=0, out_off=0):
        n = len(x) // 2
        raw_ptr = self.place(x, in_off)
        self.bout.upload(np.full(2 * n + 2 * GUARD + out_off, SENTINEL, dtype=np.float32))
        out_ptr = self.bout.ptr + 4 * (GUARD + out_off)
        ing.process_dev(raw_ptr, n, out_ptr)
        got = self.bout.download(2 * n + 2 * GUARD + out_off)
        lo, hi = got[:GUARD + out_off], got[GUARD + out_off + 2 * n:]
        assert np.all(lo == SENTINEL) and np.all(hi == SENTINEL) and len(hi) == GUARD, "a store outside out"
        return got[GUARD + out_off:GUARD + out_off + 2 * n].copy()

    def free(self):
        self.bin.free()
        self.bout.free()


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_meter(got, want, fmt, what=""):
    ints = ("n", "clipped", "nonfinite", "peak_code", "sumsq_code", "calls", "total_n", "total_clipped")
    assert [getattr(got, k) for k in ints] == [getattr(want, k) for k in ints], (what, got, want)
    assert all(isinstance(getattr(got, k), int) for k in ints)
    assert got.peak == want.peak, (what, got, want)
    if fmt == "cf32":
        assert abs(got.sumsq - want.sumsq) <= want.n * 2.0 ** -52 * want.sumsq, (what, got.sumsq, want.sumsq)
    else:
        assert got.sumsq == want.sumsq, (what, got, want)


# ---- the C entry points' refusals: no GPU, the library loaded, ctx = NULL --------------------------
class Params(ctypes.Structure):
    _fields_ = [("bits", ctypes.c_int), ("swap", ctypes.c_int), ("meter", ctypes.c_int)]


def test_create_refuses_bad_arguments_before_the_context(sdr):
    lib = sdr.load_library()
    out = ctypes.c_void_p()

    def create(dtype, bits=None, out_ref=ctypes.byref(out)):
        prm = ctypes.byref(Params(bits, 0, 1)) if bits is not None else None
        return lib.sdr_ingest_create(None, dtype, prm, out_ref)
    for args, word in (((0, None, None), "out is NULL"), ((4,), "dtype"), ((-1,), "dtype"), ((3, 1), "bits"), ((3, 17), "bits"),
                       ((3, -12), "bits"), ((2, 12), "bits"), ((1, 7), "bits"), ((0, 16), "bits"),
                       ((0,), "context is NULL"), ((1, 8), "context is NULL"), ((2,), "context is NULL"), ((2, 0), "context is NULL"),
                       ((3,), "context is NULL"), ((3, 12), "context is NULL"), ((3, 2), "context is NULL"), ((0, 32), "context is NULL")):
        assert create(*args) == -1 and word in lib.sdr_last_error().decode(), (args, lib.sdr_last_error())
    assert lib.sdr_ingest_process_dev(None, None, 8, None) == -1 and "NULL" in lib.sdr_last_error().decode()
    assert lib.sdr_ingest_run(None, None, 8, None) == -1 and "NULL" in lib.sdr_last_error().decode()
    assert lib.sdr_ingest_reset(None) == -1 and "NULL" in lib.sdr_last_error().decode()
    assert lib.sdr_ingest_meter_get(None, None) == -1 and lib.sdr_ingest_meter_dev(None, None) == -1
    lib.sdr_ingest_destroy(None)


def test_the_other_stages_still_refuse_the_raw_types(sdr):
    """SDR_IQ_S8 = 2 and SDR_IQ_S16 = 3 are sdr_ingest_create's alone"""
    lib = sdr.load_library()
    assert (sdr.SDR_IQ_S8, sdr.SDR_IQ_S16) == (2, 3)
    out = ctypes.c_void_p()
    dp = ctypes.POINTER(ctypes.c_double)
    h, f = np.ones(16) / 16.0, np.array([0.1])
    k = np.zeros(1, np.int32)
    for dtype in (2, 3):
        for rc in (lib.sdr_ddc_create(None, 1, f.ctypes.data_as(dp), h.ctypes.data_as(dp), 16, 4, dtype, ctypes.byref(out)),
                   lib.sdr_pfb_create(None, 8, 1, k.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), h.ctypes.data_as(dp), 16, 4, dtype, ctypes.byref(out)),
                   lib.sdr_spec_create(None, 64, None, 64, 1, dtype, ctypes.byref(out)),
                   lib.sdr_iqc_create(None, dtype, None, ctypes.byref(out))):
            assert rc == -1 and "dtype" in lib.sdr_last_error().decode(), (dtype, lib.sdr_last_error())
        assert lib.sdr_rx_create(None, 1, 1024, dtype, 1, ctypes.byref(out)) == -1
    for cls, kw in ((sdr.IqCorrector, {}), (sdr.Spectrum, dict(nfft=64, fs=1.0))):
        for dt in (np.int8, np.int16):
            with pytest.raises(ValueError):
                cls(iq_dtype=dt, **kw)


@gpu
def test_live_objects_refuse_bad_calls(sdr, gpu_ctx):
    """SDR_EINVAL from the C side with a live object, before any launch: the meter stays zero"""
    lib = gpu_ctx.lib
    buf = sdr.DeviceBuffer(gpu_ctx, 1 << 16)
    objs = {fmt: sdr.CaptureIngest(fmt, ctx=gpu_ctx) for fmt in FORMATS}
    try:
        h = {fmt: o._open() for fmt, o in objs.items()}
        p = buf.ptr
        for fmt, args, word in (("cs8", (p, 0, p + 32768), "n="), ("cs8", (p, 2 ** 31, p + 32768), "n="), ("cs16", (None, 8, p), "NULL"),
                                ("cs16", (p, 8, None), "NULL"), ("cu8", (p + 1, 8, p + 32768), "aligned"), ("cs8", (p + 3, 8, p + 32768), "aligned"),
                                ("cs16", (p + 2, 8, p + 32768), "aligned"), ("cf32", (p + 4, 8, p + 32768), "aligned"),
                                ("cs8", (p, 8, p + 32772), "aligned"), ("cf32", (p, 8, p + 8), "overlap"), ("cf32", (p + 8, 8, p), "overlap"),
                                ("cs8", (p, 8, p), "overlap"), ("cs16", (p + 60, 8, p), "overlap"), ("cu8", (p + 8, 8, p - 56 + 64), "overlap")):
            assert lib.sdr_ingest_process_dev(h[fmt], *args) == -1 and word in lib.sdr_last_error().decode(), (fmt, args, lib.sdr_last_error())
        for o in objs.values():
            assert o.meter() == (0, 0, 0, 0, 0, 0.0, 0.0, 0, 0, 0)
        out = ctypes.c_void_p()
        for dtype in (2, 3):                                      # the receiver looks at its context first: asked with a live one
            assert lib.sdr_rx_create(gpu_ctx.handle, 1, 1024, dtype, 1, ctypes.byref(out)) == -1 and "dtype" in lib.sdr_last_error().decode()
    finally:
        for o in objs.values():
            o.close()
        buf.free()


# ---- the device against the rule ----------------------------------------------------------------
@gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_edges_of_the_vector_and_chunk_logic(sdr, gpu_ctx, fmt):
    """every n around a vector and a chunk, the input 0 to 8 samples past a 16-byte boundary, out at
    both 8-byte phases; swap on the odd input offsets"""
    assert CHUNK == sdr.CaptureIngest.CHUNK
    b = Bench(sdr, gpu_ctx, fmt, max(EDGES))
    ing = {sw: sdr.CaptureIngest(fmt, swap=sw, ctx=gpu_ctx) for sw in (False, True)}
    try:
        for n in EDGES:
            x = random_block(fmt, n)
            want = {sw: sdr.ingest_model(x, fmt, swap=sw) for sw in (False, True)}
            assert want[False][1].clipped >= 1 and want[False][1] == want[True][1]
            for in_off in range(9):
                for out_off in (0, 2):
                    sw = bool(in_off % 2)
                    ing[sw].reset()
                    y = b.call(ing[sw], x, in_off, out_off)
                    assert same_bits(y, want[sw][0]), (n, in_off, out_off)
                    check_meter(ing[sw].meter(), want[sw][1], fmt, (n, in_off, out_off))
    finally:
        for o in ing.values():
            o.close()
        b.free()


@gpu
def test_more_samples_than_2048_minimum_chunks(sdr, gpu_ctx):
    """the chunk grows beyond CHUNK and the last one is ragged; 17 MB in, 67 MB out"""
    n = 2048 * CHUNK + 5
    x = random_block("cs8", n, seed=3)
    want, wm = sdr.ingest_model(x, "cs8")
    b = Bench(sdr, gpu_ctx, "cs8", n)
    ing = sdr.CaptureIngest("cs8", ctx=gpu_ctx)
    try:
        y = b.call(ing, x, in_off=1, out_off=2)
        assert same_bits(y, want)
        check_meter(ing.meter(), wm, "cs8")
    finally:
        ing.close()
        b.free()


@gpu
def test_64_bit_offsets(sdr, gpu_ctx):
    """2^29 + 4 099 cs8 samples that never leave the device (1 GB in, just over 4 GB out): zero but for
    a random block in the last 4 099 samples, whose output starts 2^32 bytes into out"""
    tail, n = 4099, (1 << 29) + 4099
    x = random_block("cs8", tail, seed=5)
    want, wm = sdr.ingest_model(x, "cs8")
    raw, out = sdr.DeviceBuffer(gpu_ctx, 2 * n + 16), sdr.DeviceBuffer(gpu_ctx, 8 * n)
    ing = sdr.CaptureIngest("cs8", ctx=gpu_ctx)
    try:
        raw.zero()
        raw.upload(x, offset=2 + 2 * (1 << 29))
        out.upload(np.full(64, SENTINEL, np.float32))              # must become the zeros of the first samples
        ing.process_dev(raw.ptr + 2, n, out.ptr)                   # one sample past a 16-byte boundary
        assert same_bits(out.download(2 * tail, offset=8 << 29), want)
        assert np.all(out.download(4096, offset=(8 << 29) - 4 * 4096) == 0.0) and np.all(out.download(4096) == 0.0)
        m = ing.meter()
        assert (m.n, m.clipped, m.peak_code, m.sumsq_code, m.total_n) == (n, wm.clipped, wm.peak_code, wm.sumsq_code, n)
    finally:
        ing.close()
        raw.free()
        out.free()


@gpu
@pytest.mark.parametrize("fmt,bits", (("cu8", None), ("cs8", None), ("cs16", None), ("cs16", 12), ("cs16", 2)))
def test_every_code_on_the_device(sdr, gpu_ctx, fmt, bits):
    """every value of the type: I ascending, Q descending"""
    dtype = FORMATS[fmt]
    info = np.iinfo(dtype)
    v = np.arange(info.min, info.max + 1, dtype=np.int64)
    x = np.empty(2 * len(v), dtype=dtype)
    x[0::2], x[1::2] = v.astype(dtype), v[::-1].astype(dtype)
    want, wm = sdr.ingest_model(x, fmt, bits=bits)
    width = bits or 8 * np.dtype(dtype).itemsize
    assert np.array_equal(want.astype(np.float64) * 2.0 ** (width - 1), x.astype(np.float64) - (128 if fmt == "cu8" else 0))
    ing = sdr.CaptureIngest(fmt, bits=bits, ctx=gpu_ctx)
    try:
        assert same_bits(ing.run(x), want)
        check_meter(ing.meter(), wm, fmt)
    finally:
        ing.close()


@gpu
def test_partial_width(sdr, gpu_ctx):
    """70 000 cs16 samples at -32 768: every sample adds 2^31, so the second sample of a lane already
    overflows a 32-bit partial"""
    n = 70000
    x = np.full(2 * n, -32768, dtype=np.int16)
    ing = sdr.CaptureIngest("cs16", ctx=gpu_ctx)
    try:
        y = ing.run(x)
        m = ing.meter()
        assert np.all(y == np.float32(-1.0))
        assert (m.n, m.clipped, m.peak_code, m.sumsq_code) == (n, n, 32768, n * 2 ** 31)
        assert m.peak == 1.0 and m.sumsq == 2.0 * n and m.power_dbfs == 0.0 and m.clip_share == 1.0
        check_meter(m, sdr.ingest_model(x, "cs16")[1], "cs16")
    finally:
        ing.close()


@gpu
def test_cf32_in_place(sdr, gpu_ctx):
    """out == raw, with and without swap, equals the rule; a NaN stays at its sample only; partial
    overlaps are refused"""
    n = CHUNK + 4097
    x = random_block("cf32", n, seed=2)
    nan_at = sorted(np.flatnonzero(np.isnan(x)))
    assert nan_at == [5, 9]
    b = Bench(sdr, gpu_ctx, "cf32", n)
    try:
        for sw in (False, True):
            want, wm = sdr.ingest_model(x, "cf32", swap=sw)
            ing = sdr.CaptureIngest("cf32", swap=sw, ctx=gpu_ctx)
            for off in (0, 1):                                    # 16-B aligned, and one complex sample past it
                ptr = b.place(x, off)
                ing.process_dev(ptr, n, ptr)
                got = b.bin.download(2 * n + 2 * off + 2 * (IN_GUARD // 4))
                lo = IN_GUARD // 4 + 2 * off
                assert same_bits(got[lo:lo + 2 * n].copy(), want), (sw, off)
                assert np.all(got[:lo] == np.float32(1e30)) and np.all(got[lo + 2 * n:] == np.float32(1e30))
                assert sorted(np.flatnonzero(np.isnan(got))) == [lo + (k ^ 1 if sw else k) for k in nan_at]
                check_meter(ing.meter(), sdr.ingest_model(x, "cf32", prev=wm if off else None)[1], "cf32")
            for raw_ptr, out_ptr in ((ptr, ptr + 8), (ptr + 8, ptr), (ptr, ptr + 8 * n - 8)):
                with pytest.raises(ValueError):
                    ing.process_dev(raw_ptr, n, out_ptr)
                assert gpu_ctx.lib.sdr_ingest_process_dev(ing._open(), raw_ptr, n, out_ptr) == -1
            ing.close()
    finally:
        b.free()


@gpu
@pytest.mark.parametrize("fmt", ("cs8", "cf32"))
def test_carried_totals_and_reset(sdr, gpu_ctx, fmt):
    lens = (CHUNK + 3, 17, 777)
    b = Bench(sdr, gpu_ctx, fmt, max(lens))
    ing = sdr.CaptureIngest(fmt, ctx=gpu_ctx)
    try:
        for rep in range(2):
            wm = None
            for k, n in enumerate(lens):
                x = random_block(fmt, n, seed=10 + k)
                want, wm = sdr.ingest_model(x, fmt, prev=wm)
                assert same_bits(b.call(ing, x, in_off=k, out_off=2 * (k % 2)), want)
                check_meter(ing.meter(), wm, fmt, (rep, k))
            assert (wm.calls, wm.total_n) == (3, sum(lens)) and wm.total_clipped > wm.clipped
            ing.reset()
            assert ing.meter() == (0, 0, 0, 0, 0, 0.0, 0.0, 0, 0, 0)
    finally:
        ing.close()
        b.free()


@gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_calls_and_layout(sdr, gpu_ctx, fmt):
    """the same call twice gives the same bits; run() equals process_dev(); meter=False gives the same
    out and leaves the meter alone; the meter's device copy is the struct meter() fetches"""
    n = 2 * CHUNK + 1029
    x = random_block(fmt, n, seed=4)
    want, wm = sdr.ingest_model(x, fmt)
    b = Bench(sdr, gpu_ctx, fmt, n)
    ing, bare = sdr.CaptureIngest(fmt, ctx=gpu_ctx), sdr.CaptureIngest(fmt, meter=False, ctx=gpu_ctx)
    try:
        y0 = b.call(ing, x, in_off=1)
        m0 = ing.meter()
        ing.reset()
        y1 = b.call(ing, x, in_off=1)
        m1 = ing.meter()
        assert same_bits(y0, want) and same_bits(y1, y0) and m0 == m1
        check_meter(m0, wm, fmt)
        raw = np.empty(10, dtype=np.int64)
        sdr._lib.check(gpu_ctx.lib.sdr_memcpy_d2h(gpu_ctx.handle, raw.ctypes.data, ing.meter_ptr, 80), "d2h")
        assert (list(raw[:4]), int(raw[4:5].view(np.uint64)[0]), list(raw[5:7].view(np.float64)), list(raw[7:])) == \
            (list(m0[:4]), m0.sumsq_code, [m0.peak, m0.sumsq], list(m0[7:]))
        ing.reset()
        assert same_bits(ing.run(x), want)
        check_meter(ing.meter(), wm, fmt)                           # (cf32's sumsq: another placement, another order of the sum)
        assert same_bits(ing.run(x.view(np.uint8)), want)           # raw bytes, as np.fromfile(dtype=np.uint8) reads them
        assert same_bits(b.call(bare, x, in_off=2, out_off=2), want) and same_bits(bare.run(x), want)
        assert bare.meter() == (0, 0, 0, 0, 0, 0.0, 0.0, 0, 0, 0)
    finally:
        ing.close()
        bare.close()
        b.free()


@gpu
def test_into_the_channelizer(sdr, gpu_ctx):
    """a cs16 block of a 12-bit ADC through CaptureIngest.process_dev -> Channelizer.process_dev equals
    the channelizer run on the float32 block the rule gives, bit for bit"""
    n, D, T = 1024, 4, 16
    rng = np.random.default_rng(7)
    x = rng.integers(-2048, 2048, 2 * n).astype(np.int16)
    want, _ = sdr.ingest_model(x, "cs16", bits=12)
    h = np.hanning(T + 2)[1:-1] / np.sum(np.hanning(T + 2))
    ing = sdr.CaptureIngest("cs16", bits=12, ctx=gpu_ctx)
    ch = sdr.Channelizer([0.1], 1.0, D, taps=h, ctx=gpu_ctx)
    raw, ref = sdr.DeviceBuffer.from_array(gpu_ctx, x), sdr.DeviceBuffer.from_array(gpu_ctx, want)
    mid, rows = sdr.DeviceBuffer(gpu_ctx, 8 * n), sdr.DeviceBuffer(gpu_ctx, 8 * (n // D))
    try:
        assert n // D == 256
        ing.process_dev(raw.ptr, n, mid.ptr)
        ch.process_dev(mid.ptr, n, rows.ptr, n // D)
        y = rows.download(2 * (n // D))
        ch.reset()
        ch.process_dev(ref.ptr, n, rows.ptr, n // D)
        yref = rows.download(2 * (n // D))
        assert same_bits(y, yref) and np.any(y != 0.0) and same_bits(mid.download(2 * n), want)
    finally:
        ch.close()
        ing.close()
        for d in (raw, ref, mid, rows):
            d.free()
