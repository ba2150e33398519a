"""set_timing / stage_ms of the lazily created timed blocks (IqCorrector, RowMeter: blocks.py _Timed
over csrc/sdr_ctx.h StageTimer): asking for stage times before any call opens the object and gets
the library's refusal, a ValueError like its other refusals; after set_timing(True) and one call the
named launches come back, none negative."""
import numpy as np
import pytest

gpu = pytest.mark.gpu
N = 4097                     # one workgroup's chunk and a sample: head, vectors and tail


@gpu
def test_iq_corrector_stage_ms(sdr, gpu_ctx):
    corr = sdr.IqCorrector(np.float32, ctx=gpu_ctx)
    with pytest.raises(ValueError, match="no timed call with an estimate"):
        corr.stage_ms()
    corr.set_timing(True)
    with pytest.raises(ValueError, match="no timed call with an estimate"):
        corr.stage_ms()
    x = np.random.default_rng(5).standard_normal(2 * N, dtype=np.float32)
    din, dout = sdr.DeviceBuffer.from_array(gpu_ctx, x), sdr.DeviceBuffer(gpu_ctx, 8 * N)
    corr.process_dev(din.ptr, N, dout.ptr, estimate=False)          # no estimate: not a timed call
    with pytest.raises(ValueError, match="no timed call with an estimate"):
        corr.stage_ms()
    corr.process_dev(din.ptr, N, dout.ptr)
    ms = corr.stage_ms()
    assert tuple(ms) == ("moments", "update", "apply") and all(v >= 0.0 for v in ms.values())
    corr.close()
    din.free()
    dout.free()


@gpu
def test_row_meter_stage_ms(sdr, gpu_ctx):
    meter = sdr.RowMeter(2, 100, ctx=gpu_ctx)
    with pytest.raises(ValueError, match="no timed call"):
        meter.stage_ms()
    meter.set_timing(True)
    with pytest.raises(ValueError, match="no timed call"):
        meter.stage_ms()
    x = np.random.default_rng(6).standard_normal((2, N), dtype=np.float32)
    buf = sdr.DeviceBuffer.from_array(gpu_ctx, x)
    meter.process_dev(buf.ptr, N, N)
    ms = meter.stage_ms()
    assert tuple(ms) == ("reduce", "fold") and all(v >= 0.0 for v in ms.values())
    meter.close()
    buf.free()
