#!/usr/bin/env python3
"""Time the channelizer alone (sdr_ddc_process_dev: the GEMM launch and the history update) at
16 channels x 64 taps x decim 8 on 2^25 complex samples, f32 and u8 input, with HIP events on
the context stream: warm-up, then best and median of the repeats.  The algorithmic bytes of a
launch -- the input once, nch x 8 x n / D out -- over the event time as GB/s, as a share of the
8 TB/s HBM peak, and beside the box's copy bandwidth (sdr_copy_bandwidth); the matrix-pipe time
of the same launch from its MFMA count; and the kernels' register / LDS / occupancy remarks
from the build's ddc.res.  One JSON line.

  python tools/ddc_time.py [--nch 16] [--taps 64] [--decim 8] [--log2n 25] [--reps 30] [--warmup 5]
                           [--res real-time-software-defined-radio_amd/_build/ddc.res]
"""
import argparse
import ctypes
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rtsdr  # noqa: E402

HBM_PEAK_GBS = 8000.0
CUS, SIMDS, CLOCK_GHZ, MFMA_CYCLES = 256, 4, 2.4, 16      # v_mfma_f32_16x16x32_f16 back to back: ~16 cycles per SIMD


def kernel_resources(path):
    """{kernel: {VGPRs, AGPRs, LDS, Occupancy, Scratch}} of the ddc kernels from the build's remarks"""
    out, cur = {}, None
    if not os.path.exists(path):
        return out
    keys = {"VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy",
            "LDS Size [bytes/block]": "static_lds"}
    for line in open(path, errors="replace"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            m2 = re.search(r"ddc_mma_kernelILi(\d+)ELb(\d)ELb(\d)", name)
            cur = out.setdefault(f"ddc_mma_kernel<CB={m2.group(1)},{'u8' if m2.group(2) == '1' else 'f32'},"
                                 f"{'A in LDS' if m2.group(3) == '1' else 'A from L2'}>", {}) if m2 else None
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\S+)", line)
        if m and cur is not None and m.group(1).strip() in keys:
            cur[keys[m.group(1).strip()]] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nch", type=int, default=16)
    ap.add_argument("--taps", type=int, default=64)
    ap.add_argument("--decim", type=int, default=8)
    ap.add_argument("--log2n", type=int, default=25)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--res", default=os.path.join(ROOT, "real-time-software-defined-radio_amd", "_build", "ddc.res"),
                    help="the build's resource remarks of csrc/ddc.hip")
    a = ap.parse_args()
    ctx = rtsdr.get_context()
    n, D, C, T = 1 << a.log2n, a.decim, a.nch, a.taps
    M = n // D
    stride = (M + 31) // 32 * 32
    rng = np.random.default_rng(0)
    freqs = np.linspace(-0.45, 0.45, C)
    out = rtsdr.DeviceBuffer(ctx, C * stride * 8)
    res = {"nch": C, "taps": T, "decim": D, "n": n, "reps": a.reps, "warmup": a.warmup}
    KS, NT = (2 * T + 31) // 32, (C + 7) // 8
    for name, dt in (("f32", np.float32), ("u8", np.uint8)):
        if dt == np.uint8:
            iq = rng.integers(0, 256, 2 * n, dtype=np.uint8)
        else:
            iq = (0.5 * rng.standard_normal(2 * n, dtype=np.float32))
        din = rtsdr.DeviceBuffer.from_array(ctx, iq)
        del iq
        ch = rtsdr.Channelizer(freqs, 1.0, D, taps=T, iq_dtype=dt, ctx=ctx)
        tm = rtsdr.Timer(ctx)
        for _ in range(a.warmup):
            ch.process_dev(din.ptr, n, out.ptr, stride)
        ctx.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = tm.event(), tm.event()
            tm.record(e0)
            ch.process_dev(din.ptr, n, out.ptr, stride)
            tm.record(e1)
            ctx.synchronize()
            ms.append(tm.elapsed_ms(e0, e1))
        tm.close()
        ms = np.array(ms)
        nbytes = 2 * n * np.dtype(dt).itemsize + C * 8 * M
        mfmas = (M / 16) * NT * KS * (3 if dt == np.float32 else 2)
        res[name] = {"best_us": round(float(ms.min()) * 1e3, 1), "median_us": round(float(np.median(ms)) * 1e3, 1),
                     "algorithmic_bytes": int(nbytes), "gbs_best": round(nbytes / ms.min() / 1e6, 1),
                     "gbs_median": round(nbytes / float(np.median(ms)) / 1e6, 1),
                     "share_of_8tbs_best": round(nbytes / ms.min() / 1e6 / HBM_PEAK_GBS, 4),
                     "msamples_per_s_best": round(n / ms.min() / 1e3, 1),
                     "mfma_pipe_us": round(mfmas * MFMA_CYCLES / (CUS * SIMDS * CLOCK_GHZ * 1e3), 1)}
        ch.close()
        din.free()
    gbs = ctypes.c_double(0.0)
    rtsdr._lib.check(ctx.lib.sdr_copy_bandwidth(ctx.handle, 256 << 20, 20, ctypes.byref(gbs)), "sdr_copy_bandwidth")
    res["copy_gbs"] = round(gbs.value, 1)
    for name in ("f32", "u8"):
        res[name]["share_of_copy_best"] = round(res[name]["gbs_best"] / gbs.value, 4)
    res["kernels"] = kernel_resources(a.res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
