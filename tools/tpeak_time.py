#!/usr/bin/env python3
"""Time the true-peak meter (sdr_tpeak_process_dev: reduce, fold) with HIP events on the context
stream: warm-up, then best, median and p90 of the repeats, at the span shape (8 streams x 786 432
audio samples) and the band shape (96 x 3 072), two channels, BS.1770's 4 x 12 table.

Per shape, in the same run: the box's copy and read-only stream probes over the same bytes
(sdr_copy_bandwidth, sdr_read_bandwidth); LoudnessMeter on the same rows; and the composed path the
fused stage replaces -- RowResampler(2 S, 4, 1, taps = the table's prototype, complex=False) into a
scratch buffer of four times the rows, then RowMeter on that buffer -- its two parts apart and
together.  `composed_over_fused` is the composed path's best time over the fused stage's.  The
meter's launches are timed apart in calls of their own (sdr_tpeak_set_timing).  Before anything is
timed the segments and records are compared with rtsdr.TruePeakModel for equality, and the composed
path's peak with the fused one (float32 chains against float64: 1e-5).  One JSON line.

  python tools/tpeak_time.py [--reps 30] [--warmup 5] [--out profiles/tpeak/tpeak_time.json]
                             [--res real-time-software-defined-radio_amd/_build/tpeak.res]
"""
import argparse

import numpy as np

import _blocktime as bt
from _blocktime import rtsdr
from sos_time import make_rows, timed

SHAPES = (("span", 8, 786432), ("band", 96, 3072))
SEGMENT = 4800


def verify(ctx, rows, p0, p1):
    S, n = rows[0].shape
    cap = max(4, n // SEGMENT + 1)
    meter = rtsdr.TruePeakMeter(S, 2, cap=cap, ctx=ctx)
    meter.process_dev(p0, p1, n, n)
    first, pk, sp = meter.segments()
    rec = meter.records()
    meter.close()
    model = rtsdr.TruePeakModel(S, 2).process(rows)
    want = model.records()
    if first != 0 or not np.array_equal(pk, model.peaks()) or not np.array_equal(sp, model.sample_peaks()):
        raise SystemExit("segments differ from the model")
    if not all(np.array_equal(getattr(rec, k), getattr(want, k)) for k in rec._fields):
        raise SystemExit("records differ from the model")
    return {"segments": int(pk.shape[2]), "equal_to_model": True, "total_true_peak_dbtp_row0": round(float(20 * np.log10(rec.total_peak[0].max() / 2.0)), 3)}, rec


def one_shape(ctx, name, S, n, reps, warmup):
    both = make_rows(2 * S, n)                                     # [2 S][n]: the left rows, then the right rows
    rows = [both[:S], both[S:]]
    xbuf = rtsdr.DeviceBuffer.from_array(ctx, both)
    p0, p1 = xbuf.ptr, xbuf.ptr + 4 * S * n
    up = rtsdr.DeviceBuffer(ctx, 4 * 2 * S * 4 * n)
    checked, rec = verify(ctx, rows, p0, p1)
    res = {"shape": name, "streams": S, "channels": 2, "n": n, "bytes": 4 * 2 * S * n, "verified": checked}
    tp = rtsdr.TruePeakMeter(S, 2, ctx=ctx)
    loud = rtsdr.LoudnessMeter(S, 2, ctx=ctx)
    res["true_peak_meter"] = timed(ctx, tp, lambda: tp.process_dev(p0, p1, n, n), reps, warmup)
    res["loudness_meter"] = timed(ctx, loud, lambda: loud.process_dev(p0, p1, n, n), reps, warmup)
    # the composed path: x4 rows written, then read back by the sample-peak meter
    h = rtsdr.design.true_peak_fir().astype(np.float64)
    rs = rtsdr.RowResampler(2 * S, 4, 1, taps=h.T.reshape(-1) / 4.0, complex=False, ctx=ctx)   # (the resampler scales by up)
    rm = rtsdr.RowMeter(2 * S, 4 * SEGMENT, ctx=ctx)

    def resample():
        rs.process_dev(p0, n, n, up.ptr, 4 * n)

    def meter():
        rm.process_dev(up.ptr, 4 * n, 4 * n)

    def composed():
        resample()
        meter()
    composed()
    r = rm.records()
    got = np.maximum(r.max, -r.min).astype(np.float64).reshape(2, S).T           # [S][channel]
    if not np.allclose(got, rec.peak, rtol=1e-5, atol=0):
        raise SystemExit(f"the composed path's peaks differ from the fused stage's: {got} / {rec.peak}")
    ms = bt.event_ms(ctx, (resample, meter, composed), reps, warmup)
    res["composed"] = {"resample_x4": bt.stats(ms[0], p90=True), "row_meter": bt.stats(ms[1], p90=True), "both": bt.stats(ms[2], p90=True),
                       "launches": 5, "floats_moved_per_sample": 9}
    nbytes = res["bytes"]
    copy, read = bt.copy_gbs(ctx, nbytes, reps), bt.read_gbs(ctx, nbytes, reps)
    res.update({"copy_probe_gbs": round(copy, 1), "copy_probe_us": round(2 * nbytes / copy / 1e3, 1),
                "read_probe_gbs": round(read, 1), "read_probe_us": round(nbytes / read / 1e3, 1)})
    fused = res["true_peak_meter"]["call"]["best_us"]
    res["composed_over_fused"] = round(res["composed"]["both"]["best_us"] / fused, 3)
    res["fused_over_read_probe"] = round(fused / res["read_probe_us"], 3)
    res["f64_fma_per_us"] = round(48.0 * 2 * S * n / fused, 1)
    for o in (tp, loud, rs, rm):
        o.close()
    for o in (xbuf, up):
        o.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--res", default=bt.res_path("tpeak"), help="the build's resource remarks of csrc/tpeak.hip")
    a = ap.parse_args()
    ctx = rtsdr.get_context()

    def label(m):
        return m.group(1) + (f"<up={m.group(2)},taps={m.group(3)}>" if m.group(2) else "")
    res = {"reps": a.reps, "warmup": a.warmup, "device": rtsdr.device_info(ctx.device),
           "kernels": bt.kernel_resources(a.res, r"(tpeak_reduce_kernel|tpeak_fold_kernel)(?:ILi(\d+)ELi(\d+)E)?", label,
                                          ("vgprs", "scratch", "occupancy", "static_lds")),
           "shapes": [one_shape(ctx, name, S, n, a.reps, a.warmup) for name, S, n in SHAPES]}
    bt.emit(res, a.out)


if __name__ == "__main__":
    main()
