#!/usr/bin/env python3
"""Time the capture ingest (sdr_ingest_process_dev: the conversion, and with the meter on the fold)
with HIP events on the context stream: warm-up, then best and median of the repeats, on one capture
block of 2^25 complex samples of each format -- cu8, cs8, cs16 (a 12-bit ADC's codes), cf32 -- with the
meter on and off.

In the same run the box's copy kernel moves the pass's bytes (sdr_copy_bandwidth: es n read plus 8 n
written, so 10, 10, 12 and 16 B a sample), best of its repeats: `over_copy` is the ratio of the best
times and the yardstick, never an absolute time; `meter_cost` is the metered call's best time over the
bare one's; `gbs` are algorithmic bytes over the best time.  Before anything is timed the block's
output and meter are compared with the host rule's (rtsdr.ingest_model): out bit for bit, the integer
fields and the peak exactly, cf32's sumsq within n 2^-52 of numpy's.  The capture is 2^20 samples of
four carriers plus noise at about -20 dBFS, with a few values driven onto the rails, tiled.  One
JSON line.

  python tools/ingest_time.py [--reps 20] [--warmup 3] [--log2n 25] [--out profiles/ingest/ingest_time.json]
                              [--res real-time-software-defined-radio_amd/_build/ingest.res]
"""
import argparse

import numpy as np

import _blocktime as bt
from _blocktime import rtsdr

FS = 20e6
STATIONS = ((3.1e6, 1.0), (-5.3e6, 0.5), (0.9e6, 0.3), (-7.7e6, 0.2))
TILE = 1 << 20
FORMATS = (("cu8", None), ("cs8", None), ("cs16", 12), ("cf32", None))
FMT_OF_CODE = {"0": "cf32", "1": "cu8", "2": "cs8", "3": "cs16"}          # include/sdr.h SDR_IQ_*


def make_capture(n, fmt, bits):
    rng = np.random.default_rng(0)
    m = min(n, TILE)
    t = np.arange(m) / FS
    z = sum(a * np.exp(2j * np.pi * (f * t + rng.uniform())) for f, a in STATIONS)
    z = 0.125 * (z + 0.003 * (rng.standard_normal(m) + 1j * rng.standard_normal(m)))
    x = np.empty(2 * m)
    x[0::2], x[1::2] = z.real, z.imag
    x[rng.integers(0, 2 * m, 64)] = 1.5                            # a few samples beyond full scale
    if fmt == "cf32":
        x = x.astype(np.float32)
    else:
        full = 2.0 ** ((bits or rtsdr.capture.FORMATS[fmt][1]) - 1)
        c = np.clip(np.rint(full * x), -full, full - 1)
        x = (c + 128).astype(np.uint8) if fmt == "cu8" else c.astype(rtsdr.capture.FORMATS[fmt][0])
    return np.tile(x, -(-n // m))[:2 * n]


def verify(ing, x, din, dout, n, fmt, bits):
    ing.reset()
    ing.process_dev(din.ptr, n, dout.ptr)
    got, y = ing.meter(), dout.download(2 * n)
    want, wm = rtsdr.ingest_model(x, fmt, bits=bits)
    if not np.array_equal(y.view(np.uint32), want.view(np.uint32)):
        raise SystemExit(f"{fmt}: out differs from the rule's")
    if got[:6] != wm[:6] or got[7:] != wm[7:]:
        raise SystemExit(f"{fmt}: meter {got} differs from the rule's {wm}")
    if abs(got.sumsq - wm.sumsq) > (n * 2.0 ** -52 * wm.sumsq if fmt == "cf32" else 0.0):
        raise SystemExit(f"{fmt}: sumsq {got.sumsq} outside the summation bound of {wm.sumsq}")
    return {"clipped": got.clipped, "clip_share": got.clip_share, "peak_dbfs": round(got.peak_dbfs, 3), "power_dbfs": round(got.power_dbfs, 3)}


def one_format(ctx, n, fmt, bits, reps, warmup):
    x = make_capture(n, fmt, bits)
    es = 2 * x.dtype.itemsize
    din, dout = rtsdr.DeviceBuffer.from_array(ctx, x), rtsdr.DeviceBuffer(ctx, 8 * n)
    metered, bare = rtsdr.CaptureIngest(fmt, bits=bits, ctx=ctx), rtsdr.CaptureIngest(fmt, bits=bits, meter=False, ctx=ctx)
    res = {"fmt": fmt, "bits": metered.bits, "n": n, "verified": verify(metered, x, din, dout, n, fmt, bits)}
    on, off = bt.event_ms(ctx, (lambda: metered.process_dev(din.ptr, n, dout.ptr), lambda: bare.process_dev(din.ptr, n, dout.ptr)),
                          reps, warmup)
    nbytes = (es + 8) * n
    copy = bt.copy_gbs(ctx, nbytes // 2)                            # reads and writes that many each
    res.update({"meter_on": bt.stats(on), "meter_off": bt.stats(off), "bytes": nbytes,
                "copy_probe_gbs": round(copy, 1), "copy_probe_us": round(nbytes / copy / 1e3, 1)})
    for k in ("meter_on", "meter_off"):
        res[k]["gbs"] = round(nbytes / res[k]["best_us"] / 1e3, 1)
        res[k]["over_copy"] = round(res[k]["best_us"] / res["copy_probe_us"], 3)
    res["meter_cost"] = round(res["meter_on"]["best_us"] / res["meter_off"]["best_us"], 3)
    metered.close()
    bare.close()
    din.free()
    dout.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=25)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--res", default=bt.res_path("ingest"), help="the build's resource remarks of csrc/ingest.hip")
    a = ap.parse_args()
    ctx = rtsdr.get_context()
    n = 1 << a.log2n

    def label(m):
        if m.group(2) is None:
            return m.group(1)
        return f"{m.group(1)}<{FMT_OF_CODE[m.group(2)]},{'swap' if m.group(3) == '1' else 'straight'},{'meter' if m.group(4) == '1' else 'bare'}>"
    res = {"reps": a.reps, "warmup": a.warmup, "device": rtsdr.device_info(ctx.device),
           "kernels": bt.kernel_resources(a.res, r"(ingest_(?:fold_)?kernel)(?:ILi(\d)ELb(\d)ELb(\d)E)?", label,
                                          ("vgprs", "scratch", "occupancy", "static_lds")),
           "formats": [one_format(ctx, n, fmt, bits, a.reps, a.warmup) for fmt, bits in FORMATS]}
    bt.emit(res, a.out)


if __name__ == "__main__":
    main()
