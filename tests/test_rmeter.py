"""The device-side modulation meter of rows (RowMeter, csrc/rmeter.hip) against the host rule
rtsdr.RowMeterModel (tests/test_rmeter_model.py pins that on the CPU), and the C entry points'
refusals.

What is compared, after every call (tests/rmeter_rows.py check): every integer field, the peaks (as
values), the histogram, the carried window and windows() exactly; the float64 sums within n 2^-52
sum|x| and sumsq within a relative n 2^-52 of numpy's -- the bound of any summation order, so it does
not constrain the chunking.  The rows sit between guards of 1e30 that a stray read would show in max."""
import ctypes

import numpy as np
import pytest

import rmeter_rows as rr

gpu = pytest.mark.gpu

CHUNK, SEG = 16384, 4096     # include/sdr.h SDR_RMETER_CHUNK, SDR_RMETER_SEG (RowMeter.CHUNK, RowMeter.SEG)
WINDOWS = (64, 100, 12000)
GUARD = np.float32(1e30)
PAD = 64                     # guard floats in front of the first row
NB, SCALE, LIMIT = 64, 40.0, 0.5


def lengths(W):
    return sorted({1, 2, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3, W - 1, W, W + 1})


class Params(ctypes.Structure):
    _fields_ = [("window", ctypes.c_int64), ("nbins", ctypes.c_int), ("scale", ctypes.c_float), ("limit", ctypes.c_float)]


class Rows:
    """One device allocation, reused by the calls of a test: rows placed `off` floats past a 16-byte
    boundary, `stride` floats apart, 1e30 before, between and after them."""

    def __init__(self, sdr, ctx, nfloats):
        self.buf = sdr.DeviceBuffer(ctx, 4 * (nfloats + 2 * PAD + 8))
        assert self.buf.ptr % 256 == 0

    def place(self, x, off=0, stride=None):
        S, n = x.shape
        stride = n if stride is None else stride
        host = np.full(PAD + off + S * stride + PAD, GUARD, dtype=np.float32)
        for s in range(S):
            host[PAD + off + s * stride:PAD + off + s * stride + n] = x[s]
        self.buf.upload(host)
        return self.buf.ptr + 4 * (PAD + off), stride

    def free(self):
        self.buf.free()


def state(m):
    return m.records(), m.hist(), m.windows()


def fresh(sdr, S, W):
    return state(sdr.RowMeterModel(S, W, NB, SCALE, LIMIT))


# ---- the C entry points' refusals: no GPU, the library loaded, ctx = NULL --------------------------
def test_create_refuses_bad_arguments_before_the_context(sdr):
    lib = sdr.load_library()
    out = ctypes.c_void_p()

    def create(S=1, W=64, nbins=8, scale=1.0, limit=1.0, prm=True, out_ref=ctypes.byref(out)):
        return lib.sdr_rmeter_create(None, S, ctypes.byref(Params(W, nbins, scale, limit)) if prm else None, out_ref)
    for kw, word in ((dict(out_ref=None), "out is NULL"), (dict(prm=False), "params is NULL"), (dict(S=0), "nstreams"), (dict(S=4097), "nstreams"),
                     (dict(W=63), "window"), (dict(W=2 ** 24 + 1), "window"), (dict(nbins=0), "nbins"), (dict(nbins=1025), "nbins"),
                     (dict(scale=0.0), "scale"), (dict(scale=-1.0), "scale"), (dict(scale=np.inf), "scale"), (dict(scale=np.nan), "scale"),
                     (dict(limit=np.nan), "limit"), (dict(), "context is NULL"), (dict(S=4096, W=2 ** 24, nbins=1024, limit=np.inf), "context is NULL"),
                     (dict(limit=-1.0), "context is NULL")):
        assert create(**kw) == -1 and word in lib.sdr_last_error().decode(), (kw, lib.sdr_last_error())
    assert lib.sdr_rmeter_process_dev(None, None, 8, 8) == -1 and "NULL" in lib.sdr_last_error().decode()
    assert lib.sdr_rmeter_run(None, None, 8, 8) == -1 and "NULL" in lib.sdr_last_error().decode()
    assert lib.sdr_rmeter_reset(None) == -1 and "NULL" in lib.sdr_last_error().decode()
    assert lib.sdr_rmeter_records(None, None) == -1 and lib.sdr_rmeter_hist(None, None) == -1
    assert lib.sdr_rmeter_windows(None, None, 0, None) == -1 and lib.sdr_rmeter_state_dev(None, None, None) == -1
    lib.sdr_rmeter_destroy(None)


@gpu
def test_live_object_refuses_bad_calls(sdr, gpu_ctx):
    """SDR_EINVAL from the C side with a live object, before any launch: the state stays as reset left it"""
    lib = gpu_ctx.lib
    buf = sdr.DeviceBuffer(gpu_ctx, 1 << 16)
    m, one = sdr.RowMeter(3, 100, NB, SCALE, LIMIT, ctx=gpu_ctx), sdr.RowMeter(1, 100, NB, SCALE, LIMIT, ctx=gpu_ctx)
    try:
        h, p = m._open(), buf.ptr
        for args, word in (((None, 64, 64), "NULL"), ((p, 64, 0), "n="), ((p, 64, -5), "n="), ((p, 2 ** 31, 2 ** 31), "n="),
                           ((p, 63, 64), "stride"), ((p, 0, 64), "stride"), ((p + 1, 64, 64), "aligned"), ((p + 2, 64, 64), "aligned"),
                           ((p + 7, 64, 64), "aligned")):
            assert lib.sdr_rmeter_process_dev(h, *args) == -1 and word in lib.sdr_last_error().decode(), (args, lib.sdr_last_error())
            with pytest.raises(ValueError):
                m.process_dev(*args)
        host = np.zeros((3, 64), np.float32)
        assert lib.sdr_rmeter_run(h, None, 64, 64) == -1 and lib.sdr_rmeter_run(h, host.ctypes.data, 63, 64) == -1
        assert lib.sdr_rmeter_run(h, host.ctypes.data + 2, 64, 32) == -1
        assert lib.sdr_rmeter_records(h, None) == -1 and lib.sdr_rmeter_hist(h, None) == -1
        assert lib.sdr_rmeter_windows(h, None, 4, None) == -1 and lib.sdr_rmeter_windows(h, None, -1, None) == -1
        assert lib.sdr_rmeter_state_dev(h, None, None) == -1
        assert lib.sdr_rmeter_process_dev(one._open(), p + 2, 64, 64) == -1
        rr.check(state(m), fresh(sdr, 3, 100), rr.SumBound(3))
        rr.check(state(one), fresh(sdr, 1, 100), rr.SumBound(1))
        one.process_dev(p + 4, 0, 64)                              # one stream: the stride is not looked at
        assert one.records().calls[0] == 1
    finally:
        m.close()
        one.close()
        buf.free()


# ---- the device against the rule ----------------------------------------------------------------
@gpu
@pytest.mark.parametrize("W", WINDOWS)
def test_lengths_alignments_and_guards(sdr, gpu_ctx, W):
    """every length around a wave, a chunk and a window, on 1, 3 and 8 streams, the rows 0 to 3 floats
    past a 16-byte boundary, an odd and an even stride; non-finite samples from 8 samples on"""
    assert (CHUNK, SEG) == (sdr.RowMeter.CHUNK, sdr.RowMeter.SEG)
    ns = lengths(W)
    rows = Rows(sdr, gpu_ctx, 8 * (max(ns) + 16))
    try:
        for S in (1, 3, 8):
            meter = sdr.RowMeter(S, W, NB, SCALE, LIMIT, ctx=gpu_ctx)
            for n in ns:
                x = rr.rows_of(S, n, seed=W)
                model, bound = sdr.RowMeterModel(S, W, NB, SCALE, LIMIT).process(x), rr.SumBound(S)
                bound.take(x)
                want = state(model)
                assert want[0].max.max() < 2.0
                for off in range(4):
                    for gap in (5, 8):
                        meter.reset()
                        meter.process_dev(*rows.place(x, off, n + gap + (n & 1)), n)   # n + gap + (n & 1): odd for 5, even for 8
                        rr.check(state(meter), want, bound, (S, n, off, gap))
            meter.close()
    finally:
        rows.free()


@gpu
@pytest.mark.parametrize("W", (64, 100, SEG - 1, SEG, CHUNK, CHUNK + 1, 12000))
def test_ragged_calls_against_one_call(sdr, gpu_ctx, W):
    """a 50 000-sample stream in the calls (1, 99, 100, 101, 4 095, 4 096, 4 097, 8 195, the rest): the
    rule after every call, and at the end what one call gives.  The windows on either side of the two
    kernels' threshold and of one and two chunks a window ride along."""
    S = 3
    x = rr.rows_of(S, rr.STREAM, seed=1)
    rows = Rows(sdr, gpu_ctx, S * (rr.STREAM + 8))
    meter, whole = sdr.RowMeter(S, W, NB, SCALE, LIMIT, ctx=gpu_ctx), sdr.RowMeter(S, W, NB, SCALE, LIMIT, ctx=gpu_ctx)
    model, bound, at = sdr.RowMeterModel(S, W, NB, SCALE, LIMIT), rr.SumBound(S), 0
    try:
        for k, n in enumerate(rr.RAGGED):
            part = x[:, at:at + n]
            meter.process_dev(*rows.place(part, k % 4, n + 3 + k), n)
            model.process(part)
            bound.take(part)
            rr.check(state(meter), state(model), bound, (W, k, n))
            at += n
        whole.process_dev(*rows.place(x, 1, rr.STREAM + 7), rr.STREAM)
        a, b = whole.records(), meter.records()
        for f in rr.CARRIED:
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        assert np.array_equal(whole.hist(), meter.hist()) and whole.windows().shape == (S, rr.STREAM // W, 2)
        assert np.all(np.abs(a.total_sum - b.total_sum) <= a.total_n * 2.0 ** -52 * bound.total_abs)
        assert np.all(np.abs(a.total_sumsq - b.total_sumsq) <= a.total_n * 2.0 ** -52 * a.total_sumsq)
    finally:
        meter.close()
        whole.close()
        rows.free()


@gpu
def test_non_finite_rows_and_an_empty_window(sdr, gpu_ctx):
    """rows of NaN, of +-inf, a NaN payload; one window (and one whole chunk) without a finite sample"""
    for W, n in ((64, 5 * 64 + 10), (12000, 2 * 12000 + 5)):
        x = rr.rows_of(4, n, seed=3)
        x[0, :] = np.nan
        x[1, 0::2], x[1, 1::2] = np.inf, -np.inf
        x[2, W:2 * W] = np.nan
        x.view(np.uint32)[3, W + 1] = 0x7fc00001
        rows = Rows(sdr, gpu_ctx, 4 * (n + 8))
        meter = sdr.RowMeter(4, W, NB, SCALE, LIMIT, ctx=gpu_ctx)
        model, bound = sdr.RowMeterModel(4, W, NB, SCALE, LIMIT).process(x), rr.SumBound(4)
        bound.take(x)
        try:
            meter.process_dev(*rows.place(x, 3, n + 1), n)
            got = state(meter)
            rr.check(got, state(model), bound, W)
            r = got[0]
            assert r.n[:2].tolist() == [0, 0] and r.nonfinite[:2].tolist() == [n, n] and r.max[0] == -np.inf and r.min[1] == np.inf
            assert r.empty_windows.tolist() == [n // W, n // W, 1, 0] and r.sum[1] == 0.0
            assert np.array_equal(got[2][2, 1], np.array([np.inf, -np.inf], np.float32))
        finally:
            meter.close()
            rows.free()


@gpu
@pytest.mark.parametrize("W", (64, 12000))
def test_many_windows(sdr, gpu_ctx, W):
    """more pieces than one round of the fold's lanes, more windows than a chunk holds; bins that
    collide within a round (a constant stream puts every window in bin 0)"""
    S, n = 2, 200_003
    x = rr.rows_of(S, n, seed=4)
    x[1, :] = np.float32(0.25)
    rows = Rows(sdr, gpu_ctx, S * (n + 8))
    meter = sdr.RowMeter(S, W, NB, SCALE, LIMIT, ctx=gpu_ctx)
    model, bound = sdr.RowMeterModel(S, W, NB, SCALE, LIMIT).process(x), rr.SumBound(S)
    bound.take(x)
    try:
        meter.process_dev(*rows.place(x, 2, n + 1), n)
        rr.check(state(meter), state(model), bound, W)
        assert meter.hist()[1, 0] == n // W and meter.hist()[1].sum() == n // W
    finally:
        meter.close()
        rows.free()


@gpu
def test_64_bit_row_offsets(sdr, gpu_ctx):
    """two rows 2^31 + 3 floats apart (an 8.6 GB allocation, touched at its two ends only)"""
    n, stride = 5000, (1 << 31) + 3
    x = rr.rows_of(2, n, seed=5)
    buf = sdr.DeviceBuffer(gpu_ctx, 4 * (stride + n + 2 * PAD))
    meter = sdr.RowMeter(2, 100, NB, SCALE, LIMIT, ctx=gpu_ctx)
    model, bound = sdr.RowMeterModel(2, 100, NB, SCALE, LIMIT).process(x), rr.SumBound(2)
    bound.take(x)
    try:
        for s in range(2):
            host = np.full(n + 2 * PAD, GUARD, np.float32)
            host[PAD:PAD + n] = x[s]
            buf.upload(host, offset=4 * s * stride)
        meter.process_dev(buf.ptr + 4 * PAD, stride, n)
        rr.check(state(meter), state(model), bound)
    finally:
        meter.close()
        buf.free()


@gpu
def test_reset_run_and_determinism(sdr, gpu_ctx):
    """reset returns to the state after creation; run() equals process_dev(); two fresh objects and the
    same calls give identical bits, float64 sums included; the device arrays are what records() and
    hist() fetch"""
    S, W = 3, 100
    x = rr.rows_of(S, 3 * CHUNK + 77, seed=6)
    cuts = (0, 1000, CHUNK + 1001, x.shape[1])
    rows = Rows(sdr, gpu_ctx, S * (x.shape[1] + 8))
    a, b = sdr.RowMeter(S, W, NB, SCALE, LIMIT, ctx=gpu_ctx), sdr.RowMeter(S, W, NB, SCALE, LIMIT, ctx=gpu_ctx)
    try:
        def feed(m):
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                m.process_dev(*rows.place(x[:, lo:hi], 1, hi - lo + 5), hi - lo)
            return state(m)
        ga, gb = feed(a), feed(b)
        for u, v in zip(ga[0], gb[0]):
            assert u.tobytes() == v.tobytes()
        assert ga[1].tobytes() == gb[1].tobytes() and ga[2].tobytes() == gb[2].tobytes()
        a.reset()
        rr.check(state(a), fresh(sdr, S, W), rr.SumBound(S), "reset")
        again = feed(a)
        for u, v in zip(again[0], gb[0]):
            assert u.tobytes() == v.tobytes()
        # the host path, one call of the whole stream
        a.reset()
        a.run(x)
        model, bound = sdr.RowMeterModel(S, W, NB, SCALE, LIMIT).process(x), rr.SumBound(S)
        bound.take(x)
        rr.check(state(a), state(model), bound, "run")
        rec_ptr, hist_ptr = a.state_ptr()
        raw = np.empty(S * 18, dtype=np.int64)                       # a record is 144 bytes
        sdr._lib.check(gpu_ctx.lib.sdr_memcpy_d2h(gpu_ctx.handle, raw.ctypes.data, rec_ptr, raw.nbytes), "d2h")
        raw = raw.reshape(S, 18)
        r = a.records()
        assert np.array_equal(raw[:, 0], r.n) and np.array_equal(raw[:, 4].view(np.float64), r.sum) and np.array_equal(raw[:, 16], r.wcount)
        h = np.empty((S, NB), dtype=np.uint64)
        sdr._lib.check(gpu_ctx.lib.sdr_memcpy_d2h(gpu_ctx.handle, h.ctypes.data, hist_ptr, h.nbytes), "d2h")
        assert np.array_equal(h, a.hist())
        # windows() into a smaller array: the first cap pairs, the full count reported
        counts = np.zeros(S, np.int64)
        few = np.full((S, 5, 2), 7.0, np.float32)
        sdr._lib.check(gpu_ctx.lib.sdr_rmeter_windows(a._open(), few.ctypes.data, 5, counts.ctypes.data), "windows")
        assert counts.tolist() == [x.shape[1] // W] * S and np.array_equal(few, a.windows()[:, :5])
    finally:
        a.close()
        b.close()
        rows.free()


@gpu
def test_through_the_receiver(sdr, gpu_ctx):
    """Receiver.modulation_meter and audio_meter on three synthetic stations, two blocks: the rule run
    on the rows the receiver hands out; the receiver's own outputs do not change with the meters
    attached"""
    S, B = 3, 51200
    iq = np.stack([sdr.synth.fm_iq(2 * B, seed=10 + s) for s in range(S)])
    rx, bare = (sdr.Receiver(S, B, stereo=True, iq_dtype=np.float32, ctx=gpu_ctx) for _ in range(2))
    mod, aud = rx.modulation_meter(), rx.audio_meter("left")
    fast = rx.modulation_meter(window_s=0.002, nbins=64)            # 480 samples: windows complete within a block
    try:
        fs = sdr.design.AUDIO_FS
        assert (mod.window, mod.nbins, aud.window) == (12000, 128, 2400)
        assert mod.scale == np.float32(fs / (2 * np.pi * 1e3)) and mod.limit == np.float32(2 * np.pi * 75e3 / fs)
        m_mod = sdr.RowMeterModel(S, mod.window, mod.nbins, mod.scale, mod.limit)
        m_aud = sdr.RowMeterModel(S, aud.window, aud.nbins, aud.scale, aud.limit)
        m_fast = sdr.RowMeterModel(S, fast.window, fast.nbins, fast.scale, fast.limit)
        b_mod, b_aud, b_fast = rr.SumBound(S), rr.SumBound(S), rr.SumBound(S)
        for k in range(2):
            block = iq[:, 2 * B * k:2 * B * (k + 1)]
            out = rx.process(block)
            mod.process_rx(rx)
            aud.process_rx(rx, "left")
            fast.process_rx(rx)
            ref = bare.process(block)
            assert sorted(out) == sorted(ref) and all(np.array_equal(out[n].view(np.uint32), ref[n].view(np.uint32)) for n in out)
            for name in ("demod", "left"):
                assert np.array_equal(rx.output(name).view(np.uint32), bare.output(name).view(np.uint32)), name
            for meter, model, bound, name in ((mod, m_mod, b_mod, "demod"), (aud, m_aud, b_aud, "left"), (fast, m_fast, b_fast, "demod")):
                rows = rx.output(name)
                model.process(rows)
                bound.take(rows)
                rr.check(state(meter), state(model), bound, (k, name))
        assert fast.window == 480 and fast.records().total_windows.tolist() == [2 * (B // 10) // 480] * S
        r = mod.records()
        rep = sdr.modulation_report(r, mod.hist(), fs, 1e3)
        assert r.total_n.tolist() == [2 * (B // 10)] * S and r.wcount.tolist() == [2 * (B // 10)] * S
        assert np.all(np.isfinite(rep.mpx_power_dbr)) and np.all(rep.peak_pos_hz > 0) and np.all(rep.peak_neg_hz < 0)
        with pytest.raises(ValueError):
            sdr.RowMeter(2, 100, ctx=gpu_ctx).process_rx(rx)
    finally:
        mod.close()
        aud.close()
        fast.close()
        rx.close()
        bare.close()
