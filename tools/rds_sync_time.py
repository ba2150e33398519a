#!/usr/bin/env python3
"""Time the device-side RDS block sync (sdr_rds_sync_process_links: windows, track) behind the
link bank it follows (sdr_rds_links_process_dev), and the link bank alone on the same rows in the
same run, with HIP events on the context stream -- warm-up, then best and median of the repeats.

Shapes: the C5 span shape, 8 rows x 933 888 samples of rrc_i (~19 456 bits per stream and call),
on clean rows (sigma 0.3: the sync holds, ~750 blocks per call in SYNC rounds of 64) and on noisy
ones (sigma 3.0: the bits are noise and the stage searches the whole call), and 96 rows x 3 648
samples (76 bits per stream: what a band of stations brings per reference block).  Per repeat:
a bank with no sync attached between two events, then the bank with the sync attached -- link
call, event, process_links, event -- so the sync's own time is an event interval of its own.
`ratio` is the sync stage's median over the lone link bank's.  The records of the timed rows are
compared with the host model's (RdsBlockSync on the host link layer's bits) before anything is
timed.  One JSON line.

  python tools/rds_sync_time.py [--reps 30] [--warmup 5] [--out profiles/rdssync/rds_sync_time.json]
"""
import argparse
import json
import os

import numpy as np

import _blocktime as bt
from _blocktime import rtsdr, stats
from rds_link_time import make_rows

SHAPES = ((8, 256 * 3648, 0.3), (8, 256 * 3648, 3.0), (96, 3648, 0.3))


def verify(ctx, rows, buf, bank, sync, calls=2):
    """the first calls against the host link layer + the model, stream by stream"""
    S, n = rows.shape
    links = [rtsdr.RdsLinkLayer() for _ in range(S)]
    models = [rtsdr.RdsBlockSync() for _ in range(S)]
    nrec = np.zeros(S, dtype=np.int64)
    for k in range(calls):
        bank.process_dev(buf.ptr, n, n)
        sync.process_links(bank)
        blocks, state = sync.blocks(), sync.state()
        for s in range(S):
            d = links[s].process(rows[s])["diff"]
            rec = models[s].process(d if k == 0 else d[27:])
            if blocks[s] != rec or state[s] != models[s].state():
                raise SystemExit(f"stream {s}, call {k}: device records differ from the model's")
            nrec[s] = len(rec)
    for lk in links:
        lk.close()
    return [int(v) for v in nrec], sync.state()


def shape(ctx, S, n, sigma, reps, warmup):
    rows = make_rows(S, n, sigma)
    buf = rtsdr.DeviceBuffer.from_array(ctx, rows)
    plain, bank = rtsdr.RdsLinkBank(S, n, ctx=ctx), rtsdr.RdsLinkBank(S, n, ctx=ctx)
    sync = bank.block_sync()
    nrec, state = verify(ctx, rows, buf, bank, sync)
    plain.process_dev(buf.ptr, n, n)
    plain.process_dev(buf.ptr, n, n)
    tm = rtsdr.Timer(ctx)
    alone, link, stage = [], [], []
    for r in range(warmup + reps):
        e = [tm.event() for _ in range(5)]
        tm.record(e[0])
        plain.process_dev(buf.ptr, n, n)
        tm.record(e[1])
        ctx.synchronize()
        tm.record(e[2])
        bank.process_dev(buf.ptr, n, n)
        tm.record(e[3])
        sync.process_links(bank)
        tm.record(e[4])
        ctx.synchronize()
        if r >= warmup:
            alone.append(tm.elapsed_ms(e[0], e[1]))
            link.append(tm.elapsed_ms(e[2], e[3]))
            stage.append(tm.elapsed_ms(e[3], e[4]))
    tm.close()
    res = {"nstreams": S, "n": n, "noise_sigma": sigma, "bits_per_stream": sync.max_bits,
           "records_per_stream_last_verified_call": nrec,
           "streams_synced": int(sum(st[0] for st in state)),
           "acquisitions": int(sum(st[5] for st in state)), "losses": int(sum(st[6] for st in state)),
           "link_alone": stats(alone), "link_before_sync": stats(link), "sync": stats(stage)}
    res["ratio"] = round(res["sync"]["median_us"] / res["link_alone"]["median_us"], 3)
    for b in (sync, bank, plain):
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
           "kernels": bt.kernel_resources(bt.res_path("rds_sync"), r"(rds_sync_\w+_kernel)", lambda m: m.group(1), fields),
           "shapes": [shape(ctx, S, n, sigma, a.reps, a.warmup) for S, n, sigma in SHAPES]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
