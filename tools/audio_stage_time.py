#!/usr/bin/env python3
"""Time the audio output stage alone (sdr_audio_out_dev: de-emphasis of L and R into f32 rows and
interleaved int16 PCM) at the C5 span shape -- 8 streams x 262 144 audio samples -- with HIP
events on the context stream: warm-up, then best and median of the repeats, beside the stage's
byte floor from the box's copy bandwidth (sdr_copy_bandwidth).  One JSON line.

  python tools/audio_stage_time.py [--streams 8] [--n 262144] [--reps 200] [--warmup 20]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtsdr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--tau", type=float, default=75e-6)
    a = ap.parse_args()
    ctx = rtsdr.get_context()
    lib, h = ctx.lib, ctx.handle
    S, n = a.streams, a.n
    rng = np.random.default_rng(0)
    D = rtsdr.DeviceBuffer
    left = D.from_array(ctx, (0.3 * rng.standard_normal((S, n))).astype(np.float32))
    right = D.from_array(ctx, (0.3 * rng.standard_normal((S, n))).astype(np.float32))
    lo, ro, pcm = D(ctx, 4 * S * n), D(ctx, 4 * S * n), D(ctx, 4 * S * n)
    state = D.from_array(ctx, np.zeros((S, 2)))
    b, den = rtsdr.design.deemphasis_coeffs(a.tau, 48e3)
    bp = np.ascontiguousarray(b).ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def stage(rows=True):
        rtsdr._lib.check(lib.sdr_audio_out_dev(h, left.ptr, right.ptr, n, n, S, bp, float(den[1]), state.ptr,
                                               lo.ptr if rows else None, ro.ptr if rows else None, pcm.ptr, 2 * n),
                         "sdr_audio_out_dev")

    def timed(rows):
        tm = rtsdr.Timer(ctx)
        for _ in range(a.warmup):
            stage(rows)
        ctx.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = tm.event(), tm.event()
            tm.record(e0)
            stage(rows)
            tm.record(e1)
            ms.append(tm.elapsed_ms(e0, e1))
        tm.close()
        ms = np.array(ms) * 1e3
        return {"best_us": round(float(ms.min()), 2), "median_us": round(float(np.median(ms)), 2)}

    gbs = ctypes.c_double(0.0)
    rtsdr._lib.check(lib.sdr_copy_bandwidth(h, 64 << 20, 20, ctypes.byref(gbs)), "sdr_copy_bandwidth")
    samples = 2 * S * n
    floor_bytes = samples * (4 + 4 + 2)               # each sample read once, written as f32 and as int16
    moved_bytes = samples * (4 + 4 + 4 + 2)           # the reduce launch reads the rows once more
    out = {"streams": S, "n": n, "tau": a.tau, "reps": a.reps, "warmup": a.warmup,
           "rows_and_pcm": timed(True), "pcm_only": timed(False), "copy_gbs": round(gbs.value, 1),
           "floor_bytes": floor_bytes, "floor_us": round(floor_bytes / gbs.value / 1e3, 2),
           "moved_bytes": moved_bytes, "moved_us": round(moved_bytes / gbs.value / 1e3, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
