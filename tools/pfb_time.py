#!/usr/bin/env python3
"""Time the polyphase filter bank alone (sdr_pfb_process_dev: the fold + DFT launch and the
history update) with HIP events on the context stream: warm-up, then best and median of the
repeats, at two shapes.

  shared   64 bins of M = 64, T = 256 taps, decim 8, f32, 2^25 complex samples -- the largest
           shape the channelizer (sdr_ddc) takes too: the same channel set (freqs k / 64, the
           same taps) goes through it in the same process, the two objects' timed calls
           interleaved, and `pfb_over_ddc_median` is the ratio of the medians.
  fm_band  M = 96, all 96 bins, T = 768, decim 8, 2^24 complex samples, f32 and u8.

Per timing: the algorithmic bytes of a launch -- the input once, nch x 8 x n / D out -- over the
event time as GB/s, as a share of the 8 TB/s HBM peak and of the box's copy bandwidth
(sdr_copy_bandwidth, same call), and the matrix-pipe time of the launch from its MFMA count;
the kernels' register / occupancy remarks from the build's pfb.res.  One JSON line.

  python tools/pfb_time.py [--reps 30] [--warmup 5] [--log2n-shared 25] [--log2n-fm 24]
                           [--res real-time-software-defined-radio_amd/_build/pfb.res]
"""
import argparse
import json

import numpy as np

import _blocktime as bt
from _blocktime import rtsdr

HBM_PEAK_GBS = 8000.0
CUS, SIMDS, CLOCK_GHZ, MFMA_CYCLES = 256, 4, 2.4, 16      # v_mfma_f32_16x16x32_f16 back to back: ~16 cycles per SIMD


def make_input(ctx, n, dt):
    rng = np.random.default_rng(0)
    iq = rng.integers(0, 256, 2 * n, dtype=np.uint8) if dt == np.uint8 else 0.5 * rng.standard_normal(2 * n, dtype=np.float32)
    return rtsdr.DeviceBuffer.from_array(ctx, iq)


def time_objects(ctx, objs, din, n, out, stride, reps, warmup):
    """the objects' calls interleaved: [ms per repeat] per object"""
    return bt.event_ms(ctx, [lambda o=o: o.process_dev(din.ptr, n, out.ptr, stride) for o in objs], reps, warmup)


def report(ms, n, D, nch, itemsize, mfmas):
    nbytes = 2 * n * itemsize + nch * 8 * (n // D)
    med = float(np.median(ms))
    return {"best_us": round(float(ms.min()) * 1e3, 1), "median_us": round(med * 1e3, 1), "algorithmic_bytes": int(nbytes),
            "gbs_best": round(nbytes / ms.min() / 1e6, 1), "gbs_median": round(nbytes / med / 1e6, 1),
            "share_of_8tbs_best": round(nbytes / ms.min() / 1e6 / HBM_PEAK_GBS, 4),
            "msamples_per_s_best": round(n / ms.min() / 1e3, 1), "mfmas": int(mfmas),
            "mfma_pipe_us": round(mfmas * MFMA_CYCLES / (CUS * SIMDS * CLOCK_GHZ * 1e3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n-shared", type=int, default=25)
    ap.add_argument("--log2n-fm", type=int, default=24)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--res", default=bt.res_path("pfb"),
                    help="the build's resource remarks of csrc/pfb.hip")
    a = ap.parse_args()
    ctx = rtsdr.get_context()
    res = {"reps": a.reps, "warmup": a.warmup}

    # (1) the shape both objects take
    M, T, D, n = 64, 256, 8, 1 << a.log2n_shared
    Mo = n // D
    stride = (Mo + 31) // 32 * 32
    h = rtsdr.design.pfb_coeffs(M, T // M)
    out = rtsdr.DeviceBuffer(ctx, M * stride * 8)
    din = make_input(ctx, n, np.float32)
    fb = rtsdr.FilterBank(M, 1.0, D, taps=h, ctx=ctx)
    ch = rtsdr.Channelizer(fb.freqs_hz, 1.0, D, taps=h, ctx=ctx)
    ms_fb, ms_ch = time_objects(ctx, [fb, ch], din, n, out, stride, a.reps, a.warmup)
    cols = Mo / 16
    res["shared"] = {"nbins": M, "nch": M, "taps": T, "decim": D, "n": n,
                     "pfb": report(ms_fb, n, D, M, 4, cols * ((M + 7) // 8) * ((2 * M + 31) // 32) * 3),
                     "ddc": report(ms_ch, n, D, M, 4, cols * ((M + 7) // 8) * ((2 * T + 31) // 32) * 3)}
    res["shared"]["pfb_over_ddc_median"] = round(float(np.median(ms_fb) / np.median(ms_ch)), 4)
    fb.close()
    ch.close()
    din.free()
    out.free()

    # (2) the FM band
    M, T, D, n = 96, 768, 8, 1 << a.log2n_fm
    Mo = n // D
    stride = (Mo + 31) // 32 * 32
    out = rtsdr.DeviceBuffer(ctx, M * stride * 8)
    res["fm_band"] = {"nbins": M, "nch": M, "taps": T, "decim": D, "n": n}
    for name, dt in (("f32", np.float32), ("u8", np.uint8)):
        din = make_input(ctx, n, dt)
        fb = rtsdr.FilterBank(M, 19.2e6, D, taps=T, iq_dtype=dt, ctx=ctx)
        (ms,) = time_objects(ctx, [fb], din, n, out, stride, a.reps, a.warmup)
        res["fm_band"][name] = report(ms, n, D, M, np.dtype(dt).itemsize, (Mo / 16) * ((M + 7) // 8) * ((2 * M + 31) // 32) * 3)
        fb.close()
        din.free()
    out.free()

    gbs = bt.copy_gbs(ctx)
    res["copy_gbs"] = round(gbs, 1)
    for r in (res["shared"]["pfb"], res["shared"]["ddc"], res["fm_band"]["f32"], res["fm_band"]["u8"]):
        r["share_of_copy_best"] = round(r["gbs_best"] / gbs, 4)
    res["kernels"] = bt.kernel_resources(a.res, r"pfb_mma_kernelILi(\d+)ELb(\d)ELb(\d)", bt.mma_label("pfb_mma_kernel"),
                                         ("vgprs", "agprs", "scratch", "occupancy"))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
