#!/usr/bin/env python3
"""Time the spectrum / waterfall alone (sdr_spec_process_dev: the FFT launch and, where a row is
summed in chunks, the small second launch) with HIP events on the context stream: warm-up, then
best and median of the repeats, on one capture of 2^25 complex samples, f32 and u8.

  nfft 1024 / 4096 / 8192 at hop = nfft, navg = 0 (one row) and navg = 64 (a waterfall);
  nfft 4096 at hop = 2048 (both navg).

Per timing: the algorithmic bytes -- the capture once plus the rows out -- over the event time as
GB/s, as a share of the 8 TB/s HBM peak and of the box's read-only stream of the same byte count
(sdr_read_bandwidth, same process).  Beside it the form a user has today, timed with torch events
on the same samples already on the device: (u8: convert,) window multiply, torch.fft.fft,
abs() ** 2, mean over the row's segments; `torch_over_spec_median` is the ratio of the medians.
If torch or its FFT does not load, "torch" holds the error and only the read probe is reported
against.  The kernels' register / occupancy remarks come from the build's spectrum.res.  One
JSON line.

  python tools/spectrum_time.py [--reps 20] [--warmup 3] [--log2n 25] [--no-torch]
                                [--res real-time-software-defined-radio_amd/_build/spectrum.res]
"""
import argparse
import ctypes
import json

import numpy as np

import _blocktime as bt
from _blocktime import rtsdr

HBM_PEAK_GBS = 8000.0
SHAPES = ((1024, 1024), (4096, 4096), (8192, 8192), (4096, 2048))      # (nfft, hop)
NAVGS = (0, 64)


def torch_form(torch, t, u8, w, nfft, hop, nseg, rows, navg):
    x = (t.to(torch.float32) - 128.0) * (1.0 / 128.0) if u8 else t
    z = torch.view_as_complex(x.view(-1, 2))
    seg = z[:nseg * nfft].view(nseg, nfft) if hop == nfft else z.unfold(0, nfft, hop)
    p = torch.fft.fft(seg[:rows * navg] * w, dim=-1).abs() ** 2
    return torch.fft.fftshift(p.view(rows, navg, nfft).mean(dim=1), dim=-1) * (1.0 / float(w.sum()) ** 2)


def time_torch(torch, t, u8, w, nfft, hop, nseg, rows, navg, reps, warmup):
    for _ in range(warmup):
        y = torch_form(torch, t, u8, w, nfft, hop, nseg, rows, navg)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = torch_form(torch, t, u8, w, nfft, hop, nseg, rows, navg)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return np.array(ms), y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=25)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--res", default=bt.res_path("spectrum"),
                    help="the build's resource remarks of csrc/spectrum.hip")
    a = ap.parse_args()
    ctx = rtsdr.get_context()
    n = 1 << a.log2n
    res = {"n": n, "reps": a.reps, "warmup": a.warmup, "timings": []}
    torch = None
    if a.no_torch:
        res["torch"] = "not requested"
    else:
        try:
            import torch
            probe = torch.fft.fft(torch.ones(64, dtype=torch.complex64, device="cuda"))
            torch.cuda.synchronize()
            assert abs(float(probe[0].real) - 64.0) < 1e-3
            res["torch"] = torch.__version__
        except Exception as e:                               # torch, or its FFT library, does not load here
            torch = None
            res["torch"] = f"unavailable: {type(e).__name__}: {e}"[:300]
    read_gbs = {}
    out = rtsdr.DeviceBuffer(ctx, 4 * 8192 * (n // 1024 // 64 + 1))
    rng = np.random.default_rng(0)
    for name, dt in (("f32", np.float32), ("u8", np.uint8)):
        iq = rng.integers(0, 256, 2 * n, dtype=np.uint8) if dt == np.uint8 else 0.5 * rng.standard_normal(2 * n, dtype=np.float32)
        din = rtsdr.DeviceBuffer.from_array(ctx, iq)
        t = torch.from_numpy(iq).cuda() if torch is not None else None
        for nfft, hop in SHAPES:
            for navg in NAVGS:
                sp = rtsdr.Spectrum(nfft, 19.2e6, hop=hop, navg=navg, iq_dtype=dt, ctx=ctx)
                nseg, rows = sp.rows(n)
                (ms,) = bt.event_ms(ctx, [lambda: sp.process_dev(din.ptr, n, out.ptr)], a.reps, a.warmup)
                nbytes = iq.nbytes + rows * nfft * 4
                if nbytes not in read_gbs:
                    g = ctypes.c_double(0.0)
                    rtsdr._lib.check(ctx.lib.sdr_read_bandwidth(ctx.handle, nbytes, 20, ctypes.byref(g)), "sdr_read_bandwidth")
                    read_gbs[nbytes] = g.value
                med = float(np.median(ms))
                r = {"dtype": name, "nfft": nfft, "hop": hop, "navg": navg, "nseg": nseg, "rows": rows,
                     "best_us": round(float(ms.min()) * 1e3, 1), "median_us": round(med * 1e3, 1), "algorithmic_bytes": int(nbytes),
                     "gbs_best": round(nbytes / ms.min() / 1e6, 1), "gbs_median": round(nbytes / med / 1e6, 1),
                     "share_of_8tbs_best": round(nbytes / ms.min() / 1e6 / HBM_PEAK_GBS, 4),
                     "read_probe_gbs": round(read_gbs[nbytes], 1),
                     "read_probe_us": round(nbytes / read_gbs[nbytes] / 1e3, 1),
                     "spec_over_read_probe_best": round(float(ms.min()) * 1e6 * read_gbs[nbytes] / nbytes, 3)}
                if torch is not None:
                    try:
                        w = torch.from_numpy(sp.window.astype(np.float32)).cuda()
                        mt, y = time_torch(torch, t, dt == np.uint8, w, nfft, hop, nseg, rows, navg if navg else nseg, a.reps, a.warmup)
                        got = out.download(rows * nfft).reshape(rows, nfft)
                        r.update({"torch_best_us": round(float(mt.min()) * 1e3, 1), "torch_median_us": round(float(np.median(mt)) * 1e3, 1),
                                  "torch_over_spec_median": round(float(np.median(mt)) / med, 3),
                                  "max_rel_diff_to_torch": float(np.max(np.abs(got - y.cpu().numpy())) / np.max(got))})
                        del y, w
                    except Exception as e:
                        r["torch_error"] = f"{type(e).__name__}: {e}"[:300]
                res["timings"].append(r)
                sp.close()
        din.free()
        del t
    out.free()
    res["kernels"] = bt.kernel_resources(a.res, r"spec_kernelILi(\d+)ELb(\d)",
                                         lambda m: f"spec_kernel<nfft={1 << int(m.group(1))},{'u8' if m.group(2) == '1' else 'f32'}>",
                                         ("vgprs", "agprs", "scratch", "occupancy"))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
