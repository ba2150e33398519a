#!/usr/bin/env python3
"""Time the IQ imbalance / DC offset corrector (sdr_iqc_process_dev: moments, update, apply) with HIP
events on the context stream: warm-up, then best and median of the repeats, on one capture block of
2^25 complex samples, f32 and u8.

Per type: the whole call; the apply launch alone (estimate off); the three launches apart (events
between them, sdr_iqc_set_timing, in calls of their own); and in the same run the box's copy kernel
moving the apply pass's bytes (sdr_copy_bandwidth: 16 B a sample f32, 10 B u8) and its read-only
stream probe over the moments pass's bytes (sdr_read_bandwidth: 8 B a sample f32, 2 B u8), both best
of their repeats.  `apply_over_copy` and `moments_over_read` are the ratios of the best times; `gbs`
are algorithmic bytes over the best time.  Before anything is timed the block's moments,
coefficients and rows are compared with the host model's (rtsdr.IqBalance): u8 moments exactly, f32
moments within the summation bound, coefficients within 4 f64 ulps of the model's step 3 on the
device's moments, rows within one f32 ulp.  The capture is 2^20 samples of four FM-less carriers
plus noise with the impairment of tests/iqc_capture.py, tiled.  One JSON line.

  python tools/iqc_time.py [--reps 20] [--warmup 3] [--log2n 25] [--out profiles/iqc/iqc_time.json]
                           [--res real-time-software-defined-radio_amd/_build/iqc.res]
"""
import argparse
from importlib import import_module

import numpy as np

import _blocktime as bt
from _blocktime import rtsdr

iqb = import_module(rtsdr.IqBalance.__module__)
FS = 19.2e6
STATIONS = ((3.1e6, 1.0), (-5.3e6, 0.5), (0.9e6, 0.3), (-7.7e6, 0.2))
TILE = 1 << 20


def make_capture(n, u8):
    rng = np.random.default_rng(0)
    m = min(n, TILE)
    t = np.arange(m) / FS
    z = sum(a * np.exp(2j * np.pi * (f * t + rng.uniform())) for f, a in STATIONS)
    z = 0.3 * (z + 0.003 * (rng.standard_normal(m) + 1j * rng.standard_normal(m)))
    th = np.deg2rad(4.0)
    x = np.empty(2 * m)
    x[0::2] = z.real + 0.03
    x[1::2] = 1.06 * (z.imag * np.cos(th) + z.real * np.sin(th)) - 0.02
    x = (np.rint(128.0 * x) + 128.0).astype(np.uint8) if u8 else x.astype(np.float32)
    return np.tile(x, -(-n // m))[:2 * n]


def ulps(a, b):
    return 0.0 if a == b else abs(a - b) / float(np.spacing(max(abs(a), abs(b))))


def verify(corr, x, din, dout, n, u8):
    corr.reset()
    corr.process_dev(din.ptr, n, dout.ptr)
    st = corr.state()
    y = dout.download(2 * n)
    I, Q = iqb.as_f64_pairs(x, u8)
    model = rtsdr.IqBalance(np.uint8 if u8 else np.float32)
    model.process(x)
    ms = model.state()
    if u8:
        if st[:5] != ms[:5]:
            raise SystemExit(f"u8 moments differ from the model: {st[:5]} {ms[:5]}")
    else:
        for k, t in enumerate((I, Q, I * I, Q * Q, I * Q)):
            if abs(st[k] - ms[k]) > 2.0 ** -52 * float(np.sum(np.abs(t))):     # both sums within n 2^-53 sum|t| of the exact one
                raise SystemExit(f"f32 moment {k} outside the summation bound: {st[k]} {ms[k]}")
    want = iqb.coefficients(st[:5])
    worst = max(ulps(g, w) for g, w in zip(st[5:9], want))
    if worst > 4:
        raise SystemExit(f"coefficients {worst} ulps from the model's step 3")
    ref = iqb.apply(I, Q, st[5:9])
    if not np.all(np.abs(y.astype(np.float64) - ref) <= np.spacing(np.abs(ref))):
        raise SystemExit("rows more than one f32 ulp from the model's")
    return {"c1": st.c1, "c2": st.c2, "dI": st.dI, "dQ": st.dQ, "image_db": round(st.image_db, 2), "coeff_ulps": worst,
            "rows_differing_share": float(np.mean(y != ref))}


def one_type(ctx, n, u8, reps, warmup):
    dt = np.uint8 if u8 else np.float32
    es = 2 if u8 else 8
    x = make_capture(n, u8)
    din, dout = rtsdr.DeviceBuffer.from_array(ctx, x), rtsdr.DeviceBuffer(ctx, 8 * n)
    corr = rtsdr.IqCorrector(dt, ctx=ctx)
    res = {"dtype": "u8" if u8 else "f32", "n": n, "verified": verify(corr, x, din, dout, n, u8)}
    whole, apply_only = bt.event_ms(ctx, (lambda: corr.process_dev(din.ptr, n, dout.ptr),
                                          lambda: corr.process_dev(din.ptr, n, dout.ptr, estimate=False)), reps, warmup)
    corr.set_timing(True)
    parts = {"moments": [], "update": [], "apply": []}
    for _ in range(reps):
        corr.process_dev(din.ptr, n, dout.ptr)
        for k, v in corr.stage_ms().items():
            parts[k].append(v)
    corr.set_timing(False)
    apply_bytes, moments_bytes = (es + 8) * n, es * n
    copy_gbs = bt.copy_gbs(ctx, apply_bytes // 2, reps)                            # reads and writes that many each
    read_gbs = bt.read_gbs(ctx, moments_bytes, reps)
    res.update({"call": bt.stats(whole), "apply_only": bt.stats(apply_only), "launches": {k: bt.stats(v) for k, v in parts.items()},
                "apply_bytes": apply_bytes, "moments_bytes": moments_bytes, "call_bytes": apply_bytes + moments_bytes,
                "copy_probe_gbs": round(copy_gbs, 1), "copy_probe_us": round(apply_bytes / copy_gbs / 1e3, 1),
                "read_probe_gbs": round(read_gbs, 1), "read_probe_us": round(moments_bytes / read_gbs / 1e3, 1)})
    res["apply_gbs"] = round(apply_bytes / res["apply_only"]["best_us"] / 1e3, 1)
    res["moments_gbs"] = round(moments_bytes / res["launches"]["moments"]["best_us"] / 1e3, 1)
    res["call_gbs"] = round(res["call_bytes"] / res["call"]["best_us"] / 1e3, 1)
    res["apply_over_copy"] = round(res["apply_only"]["best_us"] / res["copy_probe_us"], 3)
    res["moments_over_read"] = round(res["launches"]["moments"]["best_us"] / res["read_probe_us"], 3)
    corr.close()
    din.free()
    dout.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=25)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--res", default=bt.res_path("iqc"), help="the build's resource remarks of csrc/iqc.hip")
    a = ap.parse_args()
    ctx = rtsdr.get_context()
    n = 1 << a.log2n
    res = {"reps": a.reps, "warmup": a.warmup, "device": rtsdr.device_info(ctx.device),
           "kernels": bt.kernel_resources(a.res, r"(iqc_\w+_kernel)(?:ILb(\d)E(?:Lb(\d)E)?)?",
                                          lambda m: m.group(1) + ("" if m.group(2) is None else "<u8>" if m.group(2) == "1" else "<f32>")
                                          + ("" if m.group(3) is None else ",out16" if m.group(3) == "1" else ",out8"),
                                          ("vgprs", "scratch", "occupancy", "static_lds")),
           "types": [one_type(ctx, n, u8, a.reps, a.warmup) for u8 in (False, True)]}
    bt.emit(res, a.out)


if __name__ == "__main__":
    main()
