#!/usr/bin/env python3
"""Time the device-side RDS carrier phase stage (sdr_rds_carrier_process_dev: moments, track,
rotate, finish) and, in the same run, the symbol clock bank on the stage's rows
(sdr_rds_clock_process_dev) and a device-to-device copy that moves the stage's bytes -- the stage
reads 8 B and writes 4 B per sample, the copy reads 6 B and writes 6 B per sample -- with HIP events
on the context stream: warm-up, then best and median of the repeats.

Shapes: the C5 span shape, 8 rows x 933 888 samples of rrc_i and rrc_q (1 216 segments per stream
and call), and 96 rows x 3 648 samples (4 or 5 segments per stream: what a band of stations brings
per reference block).  The rows are tools/rds_link_time.py's, stream s turned by 20 + 40 s degrees
and 30 (s mod 5 - 2) degrees/s, noise sigma 0.3 on each branch.  Per repeat: carrier | clock | copy,
each between two events.  `vs_clock` is the stage's median over the clock bank's, `vs_copy` over the
copy's; `gbs` the 12 B per sample over the stage's median.  The rows, state and moments of the
timed rows are compared with the host model's (RdsCarrierPhase) before anything is timed.  One JSON
line.

  python tools/rds_carrier_time.py [--reps 30] [--warmup 5] [--out profiles/rdscarrier/rds_carrier_time.json]
"""
import argparse
import json
import os

import numpy as np

import _blocktime as bt
from _blocktime import rtsdr, stats
from rds_link_time import make_rows

SHAPES = ((8, 256 * 3648), (96, 3648))
SIGMA = 0.3


def make_pairs(S, n):
    x = make_rows(S, n, 0.0).astype(np.float64)
    t = np.arange(n) / 57_000.0
    i, q = np.empty((S, n), dtype=np.float32), np.empty((S, n), dtype=np.float32)
    for s in range(S):
        th = np.deg2rad(20.0 + 40.0 * s + 30.0 * (s % 5 - 2) * t)
        rng = np.random.default_rng(500 + s)
        i[s] = x[s] * np.cos(th) + rng.normal(0.0, SIGMA, n)
        q[s] = x[s] * np.sin(th) + rng.normal(0.0, SIGMA, n)
    return i, q


def verify(i, q, bi, bq, bank, calls=2):
    """the first calls against the model, stream by stream"""
    S, n = i.shape
    models = [rtsdr.RdsCarrierPhase() for _ in range(S)]
    for k in range(calls):
        bank.process_dev(bi.ptr, bq.ptr, n, n)
        rows, state, moments = bank.rows(), bank.state(), bank.moments()
        for s in range(S):
            y = models[s].process(i[s], q[s])
            if not np.array_equal(rows[s], y, equal_nan=True) or state[s] != models[s].state() or moments[s] != models[s].moments():
                raise SystemExit(f"stream {s}, call {k}: the device differs from the model")
    return state


def shape(ctx, S, n, reps, warmup):
    i, q = make_pairs(S, n)
    bi, bq = rtsdr.DeviceBuffer.from_array(ctx, i), rtsdr.DeviceBuffer.from_array(ctx, q)
    bank = rtsdr.RdsCarrierBank(S, n, ctx=ctx)
    clock = bank.clock()
    state = verify(i, q, bi, bq, bank)
    half = 6 * S * n                                               # the copy: 6 B read and 6 B written per sample
    src, dst = rtsdr.DeviceBuffer(ctx, half), rtsdr.DeviceBuffer(ctx, half)
    src.zero()
    chains = (lambda: bank.process_dev(bi.ptr, bq.ptr, n, n),
              lambda: clock.process_dev(bank.rows_ptr, n, bank.rows_stride),
              lambda: rtsdr._lib.check(ctx.lib.sdr_memcpy_d2d(ctx.handle, dst.ptr, src.ptr, half), "sdr_memcpy_d2d"))
    ms = bt.event_ms(ctx, chains, reps, warmup)
    res = {"nstreams": S, "n": n, "noise_sigma": SIGMA, "segments_per_call": n // 768, "bytes_per_call": 12 * S * n,
           "kappa": [int(st[2]) for st in state][:8], "steps": int(sum(st[3] + st[4] for st in state)),
           "carrier": stats(ms[0]), "clock": stats(ms[1]), "copy": stats(ms[2])}
    res["vs_clock"] = round(res["carrier"]["median_us"] / res["clock"]["median_us"], 3)
    res["vs_copy"] = round(res["carrier"]["median_us"] / res["copy"]["median_us"], 3)
    res["gbs"] = round(12 * S * n / (res["carrier"]["median_us"] * 1e-6) / 1e9, 1)
    res["copy_gbs"] = round(12 * S * n / (res["copy"]["median_us"] * 1e-6) / 1e9, 1)
    for b in (clock, bank):
        b.close()
    for b in (src, dst, bi, bq):
        b.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    ctx = rtsdr.get_context()
    fields = ("vgprs", "scratch", "occupancy", "static_lds")
    res = {"reps": a.reps, "warmup": a.warmup, "device": rtsdr.device_info(ctx.device),
           "kernels": bt.kernel_resources(bt.res_path("rds_carrier"), r"(rds_carrier_\w+_kernel)", lambda m: m.group(1), fields),
           "shapes": [shape(ctx, S, n, a.reps, a.warmup) for S, n in SHAPES]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
