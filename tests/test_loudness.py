"""The device-side loudness meter (LoudnessMeter, csrc/sos.hip) against the host rule
rtsdr.LoudnessModel (tests/test_sos_model.py pins that on the CPU).

What is compared: the number of completed segments and the index of the first kept exactly; every
segment energy within a relative n_seg 2^-52 + 2 2^-24 of the model's.  Meter and model both square
the float64 output of the K-weighting, not a row rounded to float32.  n_seg 2^-52 is the bound between
any two summation orders of the segment's non-negative squares (as the sums of tests/rmeter_rows.py);
2 2^-24, the allowance of a float32 rounding of the squared value, covers what the device's filter
output may differ from scipy's by (tests/test_sos.py bounds that by parts in 10^13 of the gain)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FS = 48000.0
S = 3
CALLS = (1, 1024, 3072, 4799, 4800, 4801, 2 * 4800 + 7, 1024, 1, 3072, 4801, 4799)


def rows_of(channels, n, seed=0):
    rng = np.random.default_rng([seed, channels, n])
    t = np.arange(n)
    return [(0.3 * rng.standard_normal((S, n)) + 0.5 * np.sin(2 * np.pi * t / 48.1 + np.arange(S)[:, None] + ch)).astype(np.float32)
            for ch in range(channels)]


def check(meter, model, what=""):
    first, e = meter.segments()
    want = model.energies()
    total = want.shape[2]
    assert e.dtype == np.float64 and e.shape == (meter.nstreams, meter.channels, min(total, meter.cap)), (what, e.shape, total)
    assert first == total - e.shape[2], (what, first, total)
    w = want[:, :, first:]
    rel = meter.segment * 2.0 ** -52 + 2 * 2.0 ** -24
    share = float(np.max(np.abs(e - w) / (rel * w))) if e.size else 0.0
    assert share <= 1.0, (what, share)
    return share


@pytest.mark.parametrize("channels", (1, 2))
@pytest.mark.parametrize("segment", (2048, 4800))
def test_ragged_calls_against_the_model(sdr, gpu_ctx, segment, channels):
    """call lengths around a tile and a segment mixed in one stream, the rows 0 to 3 floats past a
    16-byte boundary, between guards of 1e30 that would show in a sum"""
    n_all = sum(CALLS)
    rows = rows_of(channels, n_all, seed=segment)
    meter = sdr.LoudnessMeter(S, channels, segment=segment, cap=64, ctx=gpu_ctx)
    model = sdr.LoudnessModel(S, channels, segment=segment)
    stride = max(CALLS) + 9
    buf = sdr.DeviceBuffer(gpu_ctx, 4 * (2 * S * stride + 2 * 64 + 16))
    worst, lo = 0.0, 0
    try:
        for i, n in enumerate(CALLS):
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
            worst = max(worst, check(meter, model, (segment, channels, i, n)))
            assert np.array_equal(buf.download(host.size).view(np.uint32), host.view(np.uint32))
        assert model.energies().shape[2] == n_all // segment >= 4
        print(f"\nloudness segment {segment}, {channels} ch: worst share of the bound {worst:.3g}")
        # one call of everything on a fresh state gives segments within the same bound
        meter.reset()
        assert meter.segments()[1].shape[2] == 0 and meter.segments()[0] == 0
        meter.run(rows)
        check(meter, model, "one call")
    finally:
        meter.close()
        buf.free()


def test_the_ring_keeps_the_latest_cap_segments(sdr, gpu_ctx):
    rows = rows_of(1, 11 * 2048 + 100, seed=3)
    meter, model = sdr.LoudnessMeter(S, 1, segment=2048, cap=4, ctx=gpu_ctx), sdr.LoudnessModel(S, 1, segment=2048)
    try:
        for lo, hi in ((0, 3000), (3000, 3001), (3001, 9000), (9000, 11 * 2048 + 100)):
            meter.run([rows[0][:, lo:hi]])
            model.process([rows[0][:, lo:hi]])
            check(meter, model, (lo, hi))
        first, e = meter.segments()
        assert first == 7 and e.shape == (S, 1, 4)
        ring, open_ = meter.state_ptr()
        assert ring and open_
        meter.reset()
        model.reset()
        meter.run([rows[0][:, :5000]])
        model.process([rows[0][:, :5000]])
        assert meter.segments()[0] == 0 and check(meter, model, "after reset") <= 1.0
    finally:
        meter.close()


def test_segments_longer_than_64_tiles(sdr, gpu_ctx):
    """a segment of more than 64 tiles is folded by the whole wave, not by a lane: the same rule"""
    seg = 64 * 2048 + 8
    rows = rows_of(2, 2 * seg + 100, seed=5)
    meter, model = sdr.LoudnessMeter(S, 2, segment=seg, cap=4, ctx=gpu_ctx), sdr.LoudnessModel(S, 2, segment=seg)
    try:
        for lo, hi in ((0, seg - 1), (seg - 1, seg + 3000), (seg + 3000, 2 * seg + 100)):
            meter.run([r[:, lo:hi] for r in rows])
            model.process([r[:, lo:hi] for r in rows])
            check(meter, model, (lo, hi))
        assert meter.segments()[1].shape == (S, 2, 2)
    finally:
        meter.close()


def test_full_scale_sine_end_to_end(sdr, gpu_ctx):
    """BS.1770's calibration through run(): a 0 dBFS 997 Hz sine in the left channel reads -3.01 LUFS"""
    n = int(3.5 * FS)
    x = (2.0 * np.sin(2 * np.pi * 997.0 * np.arange(n) / FS)).astype(np.float32)
    left = np.stack([x, 0.5 * x])
    meter = sdr.LoudnessMeter(2, 2, ctx=gpu_ctx)
    try:
        meter.set_timing(True)
        meter.run([left, np.zeros_like(left)])
        assert set(meter.stage_ms()) == {"reduce", "carry", "apply", "fold"}
        r = meter.report()
        assert abs(r.momentary[0] + 3.01) < 0.02 and abs(r.short_term[0] + 3.01) < 0.02 and abs(r.integrated[0] + 3.01) < 0.02, r
        assert abs(r.integrated[1] + 3.01 + 6.0206) < 0.02 and r.blocks.tolist() == [32, 32] and r.nonfinite_blocks.tolist() == [0, 0]
    finally:
        meter.close()


def test_through_the_receiver(sdr, gpu_ctx):
    """Receiver.loudness_meter on two synthetic stations, two blocks: process_rx equals process_dev on
    the rows the receiver hands out, the receiver's outputs do not change with the meter attached"""
    S2, B = 2, 51200
    iq = np.stack([sdr.synth.fm_iq(2 * B, seed=20 + s) for s in range(S2)])
    rx, bare = (sdr.Receiver(S2, B, stereo=True, deemphasis=75e-6, iq_dtype=np.float32, ctx=gpu_ctx) for _ in range(2))
    mono = sdr.Receiver(S2, B, iq_dtype=np.float32, ctx=gpu_ctx)
    meter = rx.loudness_meter(segment=2048, cap=8)
    twin = sdr.LoudnessMeter(S2, 2, segment=2048, cap=8, ctx=gpu_ctx)
    model = sdr.LoudnessModel(S2, 2, segment=2048)
    notch = rx.audio_filter(sdr.design.pilot_notch_sos())
    try:
        assert rx.loudness_rows() == ("left_de", "right_de") and mono.loudness_rows() == ("audio",) and meter.channels == 2
        assert notch.nrows == S2 and notch.K == 1
        out_buf = sdr.DeviceBuffer(gpu_ctx, 4 * S2 * 2048)
        for k in range(2):
            block = iq[:, 2 * B * k:2 * B * (k + 1)]
            out = rx.process(block)
            meter.process_rx(rx)
            (pl, stride, n), (pr, _, _) = rx.output_ptr("left_de"), rx.output_ptr("right_de")
            assert n == 1024
            twin.process_dev(pl, pr, stride, n)
            notch.process_rx(rx, "left_de", out_ptr=out_buf.ptr)
            ref = bare.process(block)
            assert sorted(out) == sorted(ref) and all(np.array_equal(out[m].view(np.uint32), ref[m].view(np.uint32)) for m in out)
            left, right = rx.output("left_de"), rx.output("right_de")
            assert np.array_equal(left.view(np.uint32), bare.output("left_de").view(np.uint32))
            model.process([left, right])
        (f0, e0), (f1, e1) = meter.segments(), twin.segments()
        assert f0 == f1 == 0 and e0.shape == (S2, 2, 1) and np.array_equal(e0, e1)
        check(meter, model, "receiver")
        with pytest.raises(ValueError):
            sdr.LoudnessMeter(3, 2, ctx=gpu_ctx).process_rx(rx)
        with pytest.raises(ValueError):
            meter.process_rx(rx, names=("left_de",))
        out_buf.free()
    finally:
        for o in (meter, twin, notch, rx, bare, mono):
            o.close()
