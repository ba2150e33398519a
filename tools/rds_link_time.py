#!/usr/bin/env python3
"""Time the device-side RDS link layer alone (sdr_rds_links_process_dev: gather, scan, frame)
with HIP events on the context stream -- warm-up, then best and median of the repeats -- at the
C5 span shapes, 8 x 933 888 and 1 x 933 888 samples of rrc_i, beside the path it replaces,
measured in the same process on the same rows: sdr_memcpy_d2h of the rows, the widening to f64
and the host layer (RdsLinkLayer) stream by stream.

Each shape with rows of coded groups at two noise levels: sigma 0.3, where nearly every block
matches (~800 events per row: the frame rule's sequential part at its longest), and 3.0, where
the bits are noise (a few dozen matches per row).  Per shape: `carried` (a call that continues
a stream) and `block0` (the first call after a reset, which also screens the start position);
the host path's copy, widen and link times (wall
clock, best of the repeats); the row bytes over the device time as GB/s; and, with --span-ms, the
stage against the span's own GPU time (bench.py --workload c5 on the same box).  The events of
the timed rows are compared with the host layer's before anything is timed.  One JSON line.

  python tools/rds_link_time.py [--reps 30] [--warmup 5] [--span-ms 8:0.83,1:0.21] [--out FILE]
"""
import argparse
import json
import os
import time

import numpy as np

import _blocktime as bt
from _blocktime import rtsdr

N = 256 * 3648                     # a C5 span's rrc_i row: 256 blocks of 3648 samples


def make_rows(S, n, sigma):
    """coded RDS groups as half-sine symbols plus noise (the rows of tests/test_rds_links.py);
    at sigma = 0.3 nearly every block matches (~800 events per row), at 3.0 the bits are noise
    (~4 matches per 1024 windows)"""
    pulse = np.sin(np.pi * (np.arange(24) + 0.5) / 24)
    rows = np.empty((S, n), dtype=np.float32)
    for s in range(S):
        sym = rtsdr.synth.rds_symbols(n // 48 + 2, seed=s)[:n // 24]
        x = (sym[:, None] * pulse).ravel()
        rows[s] = x + np.random.default_rng(100 + s).normal(0, sigma, n)
    return rows


def event_times(ctx, call, reps, warmup, before=None):
    (ms,) = bt.event_ms(ctx, [call], reps, warmup, before)
    return bt.stats(ms)


def wall_best(fn, reps):
    best, out = float("inf"), None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3, out


def shape(ctx, S, n, sigma, reps, warmup, span_ms):
    rows = make_rows(S, n, sigma)
    buf = rtsdr.DeviceBuffer.from_array(ctx, rows)
    bank = rtsdr.RdsLinkBank(S, n, ctx=ctx)
    # the same answer first: one block-0 call and one carried call against the host layer
    links = [rtsdr.RdsLinkLayer() for _ in range(S)]
    for _ in range(2):
        bank.process_dev(buf.ptr, n, n)
        ev, status = bank.events()
        for s in range(S):
            ref = links[s].process(rows[s])["events"]
            if status[s] or [e[:3] for e in ev[s]] != ref:
                raise SystemExit(f"stream {s}: device events differ from the host layer's")
    n_events = [int(c) for c in bank.counts]
    res = {"nstreams": S, "n": n, "noise_sigma": sigma, "row_bytes": int(rows.nbytes), "events_per_stream": n_events,
           "carried": event_times(ctx, lambda: bank.process_dev(buf.ptr, n, n), reps, warmup),
           "block0": event_times(ctx, lambda: bank.process_dev(buf.ptr, n, n), reps, warmup, before=bank.reset)}
    res["carried"]["gbs_best"] = round(rows.nbytes / res["carried"]["best_us"] / 1e3, 1)
    # the path it replaces: the rows to the host, widened, through the host layer
    host = np.empty_like(rows)

    def d2h():
        rtsdr._lib.check(ctx.lib.sdr_memcpy_d2h(ctx.handle, host.ctypes.data, buf.ptr, host.nbytes), "sdr_memcpy_d2h")
    hreps = max(3, reps // 5)
    copy_ms, _ = wall_best(d2h, hreps)
    widen_ms, wide = wall_best(lambda: host.astype(np.float64), hreps)
    link_ms, _ = wall_best(lambda: [lk.process(wide[s]) for s, lk in enumerate(links)], hreps)
    events_ms, _ = wall_best(bank.events, hreps)
    res["host_path"] = {"d2h_us": round(copy_ms * 1e3, 1), "widen_us": round(widen_ms * 1e3, 1),
                        "link_us": round(link_ms * 1e3, 1), "total_us": round((copy_ms + widen_ms + link_ms) * 1e3, 1),
                        "d2h_gbs": round(rows.nbytes / copy_ms / 1e6, 1)}
    res["events_fetch_us"] = round(events_ms * 1e3, 1)      # sdr_rds_links_events + the Python lists, wall clock
    res["device_over_d2h_best"] = round(res["carried"]["best_us"] / (copy_ms * 1e3), 4)
    if S in span_ms:
        res["span_ms"] = span_ms[S]
        res["share_of_span_median"] = round(res["carried"]["median_us"] / 1e3 / span_ms[S], 4)
    for lk in links:
        lk.close()
    bank.close()
    buf.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--span-ms", default="", help="the C5 span's GPU time per stream count, e.g. 8:0.83,1:0.21")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    span_ms = {int(k): float(v) for k, v in (kv.split(":") for kv in a.span_ms.split(",") if kv)}
    ctx = rtsdr.get_context()
    info = rtsdr.device_info(ctx.device)
    res = {"reps": a.reps, "warmup": a.warmup, "device": info,
           "shapes": [shape(ctx, S, a.n, sigma, a.reps, a.warmup, span_ms) for S, sigma in ((8, 0.3), (1, 0.3), (8, 3.0), (1, 3.0))]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
