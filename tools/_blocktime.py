"""What the blocks' timing tools share (ddc_time, pfb_time, rsmp_time, spectrum_time, rspec_time,
iqc_time, ingest_time, rmeter_time, sos_time, blend_time, rds_link_time, rds_sync_time, rds_clock_time,
rds_carrier_time): the HIP-event loop, best and median (and p90) of its repeats, the parser of a
build's kernel resource remarks, the copy and read bandwidth of the box and the way a result
leaves as one JSON line."""
import ctypes
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rtsdr  # noqa: E402

_REMARKS = {"VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy",
            "LDS Size [bytes/block]": "static_lds"}


def res_path(name):
    """The build's resource remarks of csrc/<name>.hip."""
    return os.path.join(ROOT, "real-time-software-defined-radio_amd", "_build", name + ".res")


def event_ms(ctx, calls, reps, warmup, before=None):
    """Warm-up, then `reps` rounds of the calls interleaved, each between two HIP events on the
    context stream (`before`, if given, runs untimed ahead of every call): [ms per repeat] per call."""
    tm = rtsdr.Timer(ctx)
    for _ in range(warmup):
        for f in calls:
            if before:
                before()
            f()
    ctx.synchronize()
    ms = [[] for _ in calls]
    for _ in range(reps):
        for i, f in enumerate(calls):
            if before:
                before()
            e0, e1 = tm.event(), tm.event()
            tm.record(e0)
            f()
            tm.record(e1)
            ctx.synchronize()
            ms[i].append(tm.elapsed_ms(e0, e1))
    tm.close()
    return [np.array(v) for v in ms]


def stats(ms, p90=False):
    """Best and median of the repeats, in microseconds; p90: and their 90th percentile."""
    ms = np.asarray(ms)
    out = {"best_us": round(float(ms.min()) * 1e3, 1), "median_us": round(float(np.median(ms)) * 1e3, 1)}
    if p90:
        out["p90_us"] = round(float(np.percentile(ms, 90)) * 1e3, 1)
    return out


def kernel_resources(path, pattern, label, fields):
    """{label(match): {field: value}} of the kernels whose mangled name matches `pattern`, from the
    remarks file of a build; `fields` picks among vgprs, agprs, scratch, occupancy, static_lds."""
    out, cur = {}, None
    if not os.path.exists(path):
        return out
    for line in open(path, errors="replace"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            m2 = re.search(pattern, m.group(1))
            cur = out.setdefault(label(m2), {}) if m2 else None
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\S+)", line)
        if m and cur is not None and _REMARKS.get(m.group(1).strip()) in fields:
            cur[_REMARKS[m.group(1).strip()]] = int(m.group(2))
    return out


def mma_label(kernel):
    """The labeller of ddc_mma_kernel / pfb_mma_kernel <CB, U8, ALDS>."""
    return lambda m: (f"{kernel}<CB={m.group(1)},{'u8' if m.group(2) == '1' else 'f32'},"
                      f"{'A in LDS' if m.group(3) == '1' else 'A from L2'}>")


def _probe_gbs(ctx, name, nbytes, reps):
    gbs = ctypes.c_double(0.0)
    rtsdr._lib.check(getattr(ctx.lib, name)(ctx.handle, int(nbytes), int(reps), ctypes.byref(gbs)), name)
    return gbs.value


def copy_gbs(ctx, nbytes=256 << 20, reps=20):
    """GB/s (read + write) of the box's copy kernel over nbytes (sdr_copy_bandwidth), best of reps."""
    return _probe_gbs(ctx, "sdr_copy_bandwidth", nbytes, reps)


def read_gbs(ctx, nbytes, reps=20):
    """GB/s of the box's read-only stream probe over nbytes (sdr_read_bandwidth), best of reps."""
    return _probe_gbs(ctx, "sdr_read_bandwidth", nbytes, reps)


def emit(res, out=None):
    """Print the result as one JSON line; `out`: also write it to that file."""
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
