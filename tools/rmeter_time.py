#!/usr/bin/env python3
"""Time the rows' modulation meter (sdr_rmeter_process_dev: reduce, fold) with HIP events on the
context stream: warm-up, then best, median and spread of the repeats, at the span shape (8 rows x
2 621 440 samples) and the band shape (96 rows x 15 360), windows of 12 000 samples.

Per shape: the whole call; the two launches apart (events around them, sdr_rmeter_set_timing, in
calls of their own); and in the same run the box's read-only stream probe over the same bytes
(sdr_read_bandwidth: 4 B a sample), best of its repeats.  `reduce_over_read` and `call_over_read` are
ratios of the best times; `gbs` are the rows' bytes over the best time.  Before anything is timed
the call is compared with the host rule (rtsdr.RowMeterModel): integers, peaks, histogram and
windows exactly, the sums within the summation bound.  The rows are the multiplex of synth.fm_mpx
with its RDS subcarrier, a different level and carrier offset per row, one period tiled, with noise.
One JSON line.

  python tools/rmeter_time.py [--reps 30] [--warmup 5] [--window 12000] [--out profiles/rmeter/rmeter_time.json]
                              [--res real-time-software-defined-radio_amd/_build/rmeter.res]
"""
import argparse
import math

import numpy as np

import _blocktime as bt
from _blocktime import rtsdr

FS = 240e3
SHAPES = (("span", 8, 2621440), ("band", 96, 15360))
TILE = 1 << 18


def make_rows(S, n):
    rng = np.random.default_rng(0)
    m = min(n, TILE)
    base = 2 * math.pi * 75e3 / FS * rtsdr.synth.fm_mpx(m, FS, rds=True)
    x = np.empty((S, n), dtype=np.float32)
    for s in range(S):
        row = (0.5 + 0.5 * (s + 1) / S) * base + 2 * math.pi * (50.0 * s) / FS + 1e-3 * rng.standard_normal(m)
        x[s] = np.tile(row.astype(np.float32), -(-n // m))[:n]
    return x


def verify(meter, model_args, x, ptr, stride, n):
    meter.reset()
    meter.process_dev(ptr, stride, n)
    got, model = meter.records(), rtsdr.RowMeterModel(*model_args).process(x)
    want = model.records()
    for k in ("n", "nonfinite", "over", "windows", "total_windows", "empty_windows", "wcount", "max", "min", "wmax", "wmin"):
        if not np.array_equal(getattr(got, k), getattr(want, k)):
            raise SystemExit(f"{k} differs from the model: {getattr(got, k)} {getattr(want, k)}")
    if not np.array_equal(meter.hist(), model.hist()) or not np.array_equal(meter.windows(), model.windows()):
        raise SystemExit("histogram or windows differ from the model")
    ab = np.sum(np.abs(x.astype(np.float64)), axis=1)
    if np.any(np.abs(got.sum - want.sum) > n * 2.0 ** -52 * ab) or np.any(np.abs(got.sumsq - want.sumsq) > n * 2.0 ** -52 * want.sumsq):
        raise SystemExit("sums outside the summation bound")
    rep = rtsdr.modulation_report(got, meter.hist(), FS, 1e3)
    return {"windows": int(got.windows[0]), "mpx_power_dbr_row0": round(float(rep.mpx_power_dbr[0]), 3),
            "peak_pos_hz_row0": round(float(rep.peak_pos_hz[0]), 1), "carrier_offset_hz_last_row": round(float(rep.carrier_offset_hz[-1]), 3)}


def one_shape(ctx, name, S, n, window, reps, warmup):
    x = make_rows(S, n)
    buf = rtsdr.DeviceBuffer.from_array(ctx, x)
    args = (S, window, 128, np.float32(FS / (2 * math.pi * 1e3)), np.float32(2 * math.pi * 75e3 / FS))
    meter = rtsdr.RowMeter(*args, ctx=ctx)
    res = {"shape": name, "rows": S, "n": n, "window": window, "verified": verify(meter, args, x, buf.ptr, n, n)}
    (whole,) = bt.event_ms(ctx, (lambda: meter.process_dev(buf.ptr, n, n),), reps, warmup)
    meter.set_timing(True)
    parts = {"reduce": [], "fold": []}
    for _ in range(reps):
        meter.process_dev(buf.ptr, n, n)
        for k, v in meter.stage_ms().items():
            parts[k].append(v)
    meter.set_timing(False)
    nbytes = 4 * S * n
    read = bt.read_gbs(ctx, nbytes, reps)
    res.update({"call": bt.stats(whole, p90=True), "launches": {k: bt.stats(v, p90=True) for k, v in parts.items()}, "bytes": nbytes,
                "read_probe_gbs": round(read, 1), "read_probe_us": round(nbytes / read / 1e3, 1)})
    res["reduce_gbs"] = round(nbytes / res["launches"]["reduce"]["best_us"] / 1e3, 1)
    res["reduce_over_read"] = round(res["launches"]["reduce"]["best_us"] / res["read_probe_us"], 3)
    res["call_over_read"] = round(res["call"]["best_us"] / res["read_probe_us"], 3)
    meter.close()
    buf.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--window", type=int, default=12000)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--res", default=bt.res_path("rmeter"), help="the build's resource remarks of csrc/rmeter.hip")
    a = ap.parse_args()
    ctx = rtsdr.get_context()
    res = {"reps": a.reps, "warmup": a.warmup, "device": rtsdr.device_info(ctx.device),
           "kernels": bt.kernel_resources(a.res, r"(rmeter_\w+_kernel)(?:ILb(\d)E)?",
                                          lambda m: m.group(1) + ("" if m.group(2) is None else "<seg>" if m.group(2) == "1" else "<chunks>"),
                                          ("vgprs", "scratch", "occupancy", "static_lds")),
           "shapes": [one_shape(ctx, name, S, n, a.window, a.reps, a.warmup) for name, S, n in SHAPES]}
    bt.emit(res, a.out)


if __name__ == "__main__":
    main()
