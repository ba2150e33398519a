#!/usr/bin/env python3
"""Time the device-side RDS symbol clock (sdr_rds_clock_process_dev: energy, track, counts, pair,
bits, finish) alone and with the block sync behind it (RdsClockBank.feed), and in the same run the
link bank (sdr_rds_links_process_dev) alone and with its sync (process_links) on the same rows,
with HIP events on the context stream -- warm-up, then best and median of the repeats.

Shapes: the C5 span shape, 8 rows x 933 888 samples of rrc_i (1 216 segments per stream and call),
on clean rows (sigma 0.3) and on noisy ones (sigma 3.0: the bits are noise), and 96 rows x 3 648
samples (4 or 5 segments per stream: what a band of stations brings per reference block).  Per
repeat: link bank | clock | clock + feed | link bank + process_links, each between two events.
`ratio` is the clock stage's median over the lone link bank's, `ratio_with_sync` that of the two
chains.  The bits and state of the timed rows are compared with the host model's
(RdsSymbolClock) before anything is timed.  One JSON line.

  python tools/rds_clock_time.py [--reps 30] [--warmup 5] [--out profiles/rdsclock/rds_clock_time.json]
"""
import argparse
import json
import os

import numpy as np

import _blocktime as bt
from _blocktime import rtsdr, stats
from rds_link_time import make_rows

SHAPES = ((8, 256 * 3648, 0.3), (8, 256 * 3648, 3.0), (96, 3648, 0.3))


def verify(rows, buf, clock, calls=2):
    """the first calls against the model, stream by stream"""
    S, n = rows.shape
    models = [rtsdr.RdsSymbolClock() for _ in range(S)]
    for k in range(calls):
        clock.process_dev(buf.ptr, n, n)
        bits, state = clock.bits(), clock.state()
        for s in range(S):
            if not np.array_equal(bits[s], models[s].process(rows[s])) or state[s] != models[s].state():
                raise SystemExit(f"stream {s}, call {k}: the device differs from the model")
    return state


def shape(ctx, S, n, sigma, reps, warmup):
    rows = make_rows(S, n, sigma)
    buf = rtsdr.DeviceBuffer.from_array(ctx, rows)
    plain, bank = rtsdr.RdsLinkBank(S, n, ctx=ctx), rtsdr.RdsLinkBank(S, n, ctx=ctx)
    lsync = bank.block_sync()
    alone, clock = rtsdr.RdsClockBank(S, n, ctx=ctx), rtsdr.RdsClockBank(S, n, ctx=ctx)
    csync = clock.block_sync()
    state = verify(rows, buf, alone)
    clock.process_dev(buf.ptr, n, n)
    clock.process_dev(buf.ptr, n, n)
    chains = (lambda: plain.process_dev(buf.ptr, n, n),
              lambda: alone.process_dev(buf.ptr, n, n),
              lambda: (clock.process_dev(buf.ptr, n, n), clock.feed(csync)),
              lambda: (bank.process_dev(buf.ptr, n, n), lsync.process_links(bank)))
    ms = bt.event_ms(ctx, chains, reps, warmup)
    res = {"nstreams": S, "n": n, "noise_sigma": sigma, "segments_per_call": n // 768, "bits_per_stream_max": clock.max_bits,
           "phi_steps": int(sum(st[6] + st[7] for st in state)), "pairing_changes": int(sum(st[9] for st in state)),
           "clock_streams_synced": int(sum(st[0] for st in csync.state())),
           "link_streams_synced": int(sum(st[0] for st in lsync.state())),
           "link_alone": stats(ms[0]), "clock_alone": stats(ms[1]), "clock_and_sync": stats(ms[2]), "link_and_sync": stats(ms[3])}
    res["ratio"] = round(res["clock_alone"]["median_us"] / res["link_alone"]["median_us"], 3)
    res["ratio_with_sync"] = round(res["clock_and_sync"]["median_us"] / res["link_and_sync"]["median_us"], 3)
    for b in (csync, clock, alone, lsync, bank, plain):
        b.close()
    buf.free()
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
           "kernels": bt.kernel_resources(bt.res_path("rds_clock"), r"(rds_clock_\w+_kernel)", lambda m: m.group(1), fields),
           "shapes": [shape(ctx, S, n, sigma, a.reps, a.warmup) for S, n, sigma in SHAPES]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
