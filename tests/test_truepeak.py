"""The device-side true-peak meter (TruePeakMeter, csrc/tpeak.hip) against the host rule
rtsdr.TruePeakModel (tests/test_truepeak_model.py pins that on the CPU).

What is compared: everything, for equality.  An f32 x f32 product is exact in f64, so the device's
fused multiply-adds round as numpy's products and sums do, the taps are taken in the same order and
a maximum does not depend on the order it is taken in: the kept segments' true and sample peaks, the
index of the first kept and every field of the records equal the model's under np.array_equal.  No
tolerance."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S = 3
LOUDNESS_CALLS = (1, 1024, 3072, 4799, 4800, 4801, 2 * 4800 + 7, 1024, 1, 3072, 4801, 4799)   # tests/test_loudness.py CALLS
CALLS = (1, 5, 11, 12, 13) + LOUDNESS_CALLS       # in front: shorter than, equal to and one longer than the history of 11


def rows_of(channels, n, seed=0, nstreams=S):
    rng = np.random.default_rng([seed, channels, n])
    t = np.arange(n)
    return [(0.3 * rng.standard_normal((nstreams, n)) + 0.5 * np.sin(2 * np.pi * t / 48.1 + np.arange(nstreams)[:, None] + ch)).astype(np.float32)
            for ch in range(channels)]


def check(meter, model, what=""):
    first, pk, sp = meter.segments()
    want_pk, want_sp = model.peaks(), model.sample_peaks()
    total = want_pk.shape[2]
    assert pk.dtype == sp.dtype == np.float64 and pk.shape == sp.shape == (meter.nstreams, meter.channels, min(total, meter.cap)), (what, pk.shape, total)
    assert first == total - pk.shape[2], (what, first, total)
    assert np.array_equal(pk, want_pk[:, :, first:]), (what, "true peaks")
    assert np.array_equal(sp, want_sp[:, :, first:]), (what, "sample peaks")
    got, want = meter.records(), model.records()
    for k in got._fields:
        g, w = getattr(got, k), getattr(want, k)
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, k, g, w)


def ragged(sdr, gpu_ctx, calls, channels, segment, taps, seed):
    """the calls one after the other from rows 0 to 3 floats past a 16-byte boundary, between guards
    of 1e30 that must come back untouched (and that would show in any maximum); then one run of
    everything on a fresh state"""
    n_all = sum(calls)
    rows = rows_of(channels, n_all, seed=seed)
    meter = sdr.TruePeakMeter(S, channels, segment=segment, cap=64, taps=taps, ctx=gpu_ctx)
    model = sdr.TruePeakModel(S, channels, segment=segment, taps=taps)
    stride = max(calls) + 9
    buf = sdr.DeviceBuffer(gpu_ctx, 4 * (2 * S * stride + 2 * 64 + 16))
    lo = 0
    try:
        for i, n in enumerate(calls):
            off = i % 4
            host = np.full(64 + off + 2 * S * stride + 64, np.float32(1e30), dtype=np.float32)
            for ch in range(channels):
                for s in range(S):
                    at = 64 + off + (ch * S + s) * stride
                    host[at:at + n] = rows[ch][s, lo:lo + n]
            buf.upload(host)
            p0 = buf.ptr + 4 * (64 + off)
            meter.process_dev(p0, p0 + 4 * S * stride if channels == 2 else None, stride, n)
            model.process([r[:, lo:lo + n] for r in rows])
            lo += n
            check(meter, model, (segment, channels, i, n))
            assert np.array_equal(buf.download(host.size).view(np.uint32), host.view(np.uint32))
        assert model.peaks().shape[2] == n_all // segment >= 4
        meter.reset()
        assert meter.segments()[1].shape[2] == 0 and meter.segments()[0] == 0
        meter.run(rows)
        one = sdr.TruePeakModel(S, channels, segment=segment, taps=taps).process(rows)
        check(meter, one, "one call")
        assert np.array_equal(one.peaks(), model.peaks()) and np.array_equal(one.sample_peaks(), model.sample_peaks())
    finally:
        meter.close()
        buf.free()


@pytest.mark.parametrize("channels", (1, 2))
@pytest.mark.parametrize("segment", (2048, 4800))
def test_ragged_calls_against_the_model(sdr, gpu_ctx, segment, channels):
    ragged(sdr, gpu_ctx, CALLS, channels, segment, None, segment)


@pytest.mark.parametrize("shape", ((3, 7), (8, 32)))
def test_a_table_that_is_not_its_own_mirror_image(sdr, gpu_ctx, shape):
    """BS.1770's table reversed in both phases and taps is itself: a random one tells the orders apart.
    Calls around its history of taps - 1 samples in front."""
    taps = np.random.default_rng(shape).standard_normal(shape).astype(np.float32)
    assert not np.array_equal(taps, taps[::-1, ::-1])
    hl = shape[1] - 1
    ragged(sdr, gpu_ctx, (1, hl - 1, hl, hl + 1, 2, 3072, 4801, 2049, 1, 4799), 2, 2048, taps, shape[1])


def test_unit_table_reads_the_sample_peak(sdr, gpu_ctx):
    rows = rows_of(1, 5000, seed=9)
    meter = sdr.TruePeakMeter(S, 1, segment=2048, cap=4, taps=[[1.0]], ctx=gpu_ctx)
    try:
        meter.run(rows)
        first, pk, sp = meter.segments()
        assert first == 0 and pk.shape == (S, 1, 2) and np.array_equal(pk, sp)
        assert np.array_equal(sp[:, 0, 0], np.max(np.abs(rows[0][:, :2048]), axis=1).astype(np.float64))
    finally:
        meter.close()


def test_the_ring_keeps_the_latest_cap_segments(sdr, gpu_ctx):
    rows = rows_of(1, 11 * 2048 + 100, seed=3)
    meter, model = sdr.TruePeakMeter(S, 1, segment=2048, cap=4, ctx=gpu_ctx), sdr.TruePeakModel(S, 1, segment=2048)
    try:
        for lo, hi in ((0, 3000), (3000, 3001), (3001, 9000), (9000, 11 * 2048 + 100)):
            meter.run([rows[0][:, lo:hi]])
            model.process([rows[0][:, lo:hi]])
            check(meter, model, (lo, hi))
        first, pk, sp = meter.segments()
        assert first == 7 and pk.shape == sp.shape == (S, 1, 4)
        assert all(meter.state_ptr())
        meter.reset()
        model.reset()
        meter.run([rows[0][:, :5000]])
        model.process([rows[0][:, :5000]])
        assert meter.segments()[0] == 0
        check(meter, model, "after reset")
    finally:
        meter.close()


@pytest.mark.parametrize("seg", (4096 + 8, 64 * 4096 + 8))
def test_segments_longer_than_a_piece_and_than_64_pieces(sdr, gpu_ctx, seg):
    """a segment of several pieces is folded by a lane, one of more than 64 by the whole wave: the same rule"""
    rows = rows_of(2, 2 * seg + 100, seed=5)
    meter, model = sdr.TruePeakMeter(S, 2, segment=seg, cap=4, ctx=gpu_ctx), sdr.TruePeakModel(S, 2, segment=seg)
    try:
        for lo, hi in ((0, seg - 1), (seg - 1, seg + 3000), (seg + 3000, 2 * seg + 100)):
            meter.run([r[:, lo:hi] for r in rows])
            model.process([r[:, lo:hi] for r in rows])
            check(meter, model, (seg, lo, hi))
        assert meter.segments()[1].shape == (S, 2, 2)
    finally:
        meter.close()


@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_non_finite_samples(sdr, gpu_ctx, bad):
    """a non-finite sample makes up x taps values non-finite: they are counted, enter no maximum and
    touch no other row; one in the last taps - 1 samples of a call reaches the next through the history"""
    n0, n1 = 3000, 2500
    rows = rows_of(2, n0 + n1, seed=11)
    at = (1234, n0 - 4)                                            # mid-call; 4 from the end: 8 of its 12 samples are the next call's
    rows[0][1, at[0]] = bad
    rows[1][2, at[1]] = bad
    meter, model = sdr.TruePeakMeter(S, 2, segment=2048, cap=8, ctx=gpu_ctx), sdr.TruePeakModel(S, 2, segment=2048)
    clean = sdr.TruePeakModel(S, 2, segment=2048)
    try:
        for k, (lo, hi) in enumerate(((0, n0), (n0, n0 + n1))):
            meter.run([r[:, lo:hi] for r in rows])
            model.process([r[:, lo:hi] for r in rows])
            clean.process([np.where(np.isfinite(r[:, lo:hi]), r[:, lo:hi], np.float32(0.25)) for r in rows])
            check(meter, model, (bad, lo, hi))
            rec = meter.records()
            want = np.zeros((S, 2), dtype=np.int64)
            want[1, 0] = 48 if k == 0 else 0
            want[2, 1] = 4 * 4 if k == 0 else 4 * 8
            assert np.array_equal(rec.nonfinite, want), (bad, k, rec.nonfinite)
            assert np.all(np.isfinite(rec.peak)) and np.all(np.isfinite(rec.sample_peak)) and np.all(np.isfinite(rec.open_peak))
        _, pk, sp = meter.segments()
        assert np.all(np.isfinite(pk)) and np.all(np.isfinite(sp)) and np.all(pk > 0)
        untouched = np.ones((S, 2), dtype=bool)
        untouched[1, 0] = untouched[2, 1] = False
        assert np.array_equal(pk[untouched], clean.peaks()[untouched]) and np.array_equal(sp[untouched], clean.sample_peaks()[untouched])
        assert np.array_equal(meter.records().total_nonfinite, [[0, 0], [48, 0], [0, 48]])
        assert np.array_equal(meter.report().nonfinite, [0, 48, 48])
    finally:
        meter.close()


class Params(ctypes.Structure):
    _fields_ = [("up", ctypes.c_int), ("taps", ctypes.c_int), ("h", ctypes.c_void_p), ("segment", ctypes.c_int64), ("cap", ctypes.c_int)]


def test_refusals_come_before_any_device_work(sdr, gpu_ctx):
    lib = sdr.load_library()
    err = lambda: lib.sdr_last_error().decode()                     # noqa: E731
    out = ctypes.c_void_p()
    table = np.ones((8, 32), dtype=np.float32)
    nan_table = table.copy()
    nan_table[7, 31] = np.nan

    def create(S=1, channels=2, up=4, taps=12, h=None, segment=4800, cap=64, prm=True, out_ref=ctypes.byref(out), ctx=None):
        p = Params(up, taps, None if h is None else h.ctypes.data, segment, cap)
        return lib.sdr_tpeak_create(ctx, S, channels, ctypes.byref(p) if prm else None, out_ref)
    # without a context: every refusal is raised in front of the context's own
    for kw, word in ((dict(out_ref=None), "out is NULL"), (dict(prm=False), "params is NULL"), (dict(S=0), "nstreams"), (dict(S=4097), "nstreams"),
                     (dict(channels=3), "channels"), (dict(up=3), "without a table"), (dict(up=0, h=table), "up=0"), (dict(up=9, h=table), "up=9"),
                     (dict(taps=0, h=table), "taps=0"), (dict(taps=33, h=table), "taps=33"), (dict(up=8, taps=32, h=nan_table), "not finite"),
                     (dict(segment=2047), "segment"), (dict(segment=(1 << 24) + 1), "segment"), (dict(cap=3), "cap"), (dict(cap=(1 << 20) + 1), "cap"),
                     (dict(), "context is NULL")):
        assert create(**kw) == -1 and word in err(), (kw, err())
    assert lib.sdr_tpeak_process_dev(None, None, None, 8, 8) == -1 and "NULL" in err()
    assert lib.sdr_tpeak_run(None, None, None, 8, 8) == -1 and "NULL" in err()
    assert lib.sdr_tpeak_reset(None) == -1 and lib.sdr_tpeak_records(None, None) == -1 and lib.sdr_tpeak_segments(None, None, None, None, None) == -1
    assert lib.sdr_tpeak_state_dev(None, None, None, None) == -1 and lib.sdr_tpeak_set_timing(None, 1) == -1 and lib.sdr_tpeak_stage_ms(None, None) == -1
    lib.sdr_tpeak_destroy(None)
    assert create(up=0, taps=0, ctx=gpu_ctx.handle) == 0 and out.value                 # h NULL, up = taps = 0: the default table
    try:
        x = sdr.DeviceBuffer(gpu_ctx, 4 * 64)
        p = x.ptr
        for args, word in (((None, p, 8, 8), "ch0 is NULL"), ((p, None, 8, 8), "ch1"), ((p, p, 8, 0), "n=0"), ((p, p, 8, 1 << 31), "n="),
                           ((p, p, 7, 8), "stride"), ((p + 2, p, 8, 8), "aligned"), ((p, p + 1, 8, 8), "aligned")):
            assert lib.sdr_tpeak_process_dev(out, *args) == -1 and word in err(), (args, err())
        assert lib.sdr_tpeak_run(out, None, None, 8, 8) == -1 and lib.sdr_tpeak_run(out, p, None, 8, 8) == -1
        ms = (ctypes.c_float * 2)()
        assert lib.sdr_tpeak_stage_ms(out, ms) == -1 and "no timed call" in err()
        rec = np.zeros(2 * 12, dtype=np.int64)
        assert lib.sdr_tpeak_records(out, rec.ctypes.data) == 0 and not rec.any()   # no refused call left a trace
        x.free()
    finally:
        lib.sdr_tpeak_destroy(out)
    # the Python object checks its arguments before a context exists
    for kw in (dict(nstreams=0), dict(channels=3), dict(segment=2047), dict(cap=3), dict(cap=(1 << 20) + 1), dict(taps=np.ones((9, 2))),
               dict(taps=np.ones((2, 33))), dict(taps=[[np.inf]]), dict(taps=np.ones((2, 2, 2))), dict(reference=0.0)):
        with pytest.raises(ValueError):
            sdr.TruePeakMeter(**{"nstreams": 1, **kw})
    meter = sdr.TruePeakMeter(2, 2, ctx=gpu_ctx)
    for args in ((0, 8, 8, 8), (8, 0, 8, 8), (8, 8, 8, 0), (8, 8, 7, 8), (6, 8, 8, 8)):
        with pytest.raises(ValueError):
            meter.process_dev(*args)
    with pytest.raises(ValueError):
        meter.run([np.zeros((2, 8))])
    assert meter.handle is None                                      # none of it made the device object


def test_stage_names_and_a_full_scale_sine(sdr, gpu_ctx):
    """a 0 dBFS sine at fs / 4 sampled 45 degrees off its crests: the sample peak reads -3.01 dBFS, the
    true peak 0 dBTP within EBU Tech 3341's +0.2 / -0.4 dB"""
    n = 48000
    x = (2.0 * np.sin(2 * np.pi * (np.arange(n) / 4.0) + np.pi / 4)).astype(np.float32)
    meter = sdr.TruePeakMeter(2, 1, ctx=gpu_ctx)
    try:
        meter.set_timing(True)
        meter.run([np.stack([x, 0.5 * x])])
        assert set(meter.stage_ms()) == {"reduce", "fold"} and all(v >= 0 for v in meter.stage_ms().values())
        r = meter.report()
        assert abs(r.sample_peak_dbfs[0] + 3.0103) < 1e-3 and -0.4 <= r.true_peak_dbtp[0] <= 0.2 and -0.4 <= r.latest_dbtp[0] <= 0.2, r
        assert abs(r.true_peak_dbtp[1] - r.true_peak_dbtp[0] + 6.0206) < 1e-3 and r.total_true_peak_dbtp[0] == r.true_peak_dbtp[0]
        assert r.nonfinite.tolist() == [0, 0]
    finally:
        meter.close()


def test_through_the_receiver(sdr, gpu_ctx):
    """Receiver.true_peak_meter on two synthetic stereo stations, two blocks: process_rx equals
    process_dev on the rows the receiver hands out and the model on the downloaded rows; the receiver's
    outputs do not change with the meter attached"""
    S2, B = 2, 51200
    iq = np.stack([sdr.synth.fm_iq(2 * B, seed=20 + s) for s in range(S2)])
    rx, bare = (sdr.Receiver(S2, B, stereo=True, deemphasis=75e-6, iq_dtype=np.float32, ctx=gpu_ctx) for _ in range(2))
    meter = rx.true_peak_meter(segment=2048, cap=8)
    twin = sdr.TruePeakMeter(S2, 2, segment=2048, cap=8, ctx=gpu_ctx)
    model = sdr.TruePeakModel(S2, 2, segment=2048)
    try:
        assert meter.channels == 2 and meter.nstreams == S2 and meter._ctx is rx.ctx
        for k in range(2):
            block = iq[:, 2 * B * k:2 * B * (k + 1)]
            out = rx.process(block)
            meter.process_rx(rx)
            (pl, stride, n), (pr, _, _) = rx.output_ptr("left_de"), rx.output_ptr("right_de")
            assert n == 1024
            twin.process_dev(pl, pr, stride, n)
            ref = bare.process(block)
            assert sorted(out) == sorted(ref) and all(np.array_equal(out[m].view(np.uint32), ref[m].view(np.uint32)) for m in out)
            left, right = rx.output("left_de"), rx.output("right_de")
            assert np.array_equal(left.view(np.uint32), bare.output("left_de").view(np.uint32))
            assert np.array_equal(right.view(np.uint32), bare.output("right_de").view(np.uint32))
            model.process([left, right])
        a, b = meter.segments(), twin.segments()
        assert a[0] == b[0] == 0 and a[1].shape == (S2, 2, 1) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        assert all(np.array_equal(u, v) for u, v in zip(meter.records(), twin.records()))
        check(meter, model, "receiver")
        assert np.all(np.isfinite(meter.report().total_true_peak_dbtp))
        with pytest.raises(ValueError):
            sdr.TruePeakMeter(3, 2, ctx=gpu_ctx).process_rx(rx)
        with pytest.raises(ValueError):
            meter.process_rx(rx, names=("left_de",))
    finally:
        for o in (meter, twin, rx, bare):
            o.close()
