"""Digest of the full-range passes' outputs (GPU box), in the manner of tools/blocks_digest.py: for
a fixed list of small IqCorrector / CaptureIngest / RowMeter calls -- aimed at what the passes
share: the head / vector / tail split of a range at every alignment, one and many workgroups, the
grown chunk, the records' fold -- one line per call with a SHA-256 (its first 16 hex digits) of the
call's whole output buffer, guard floats included, and of the state the call leaves.  Two libraries
compute the same thing when their outputs are identical line for line (SDR_LIB selects the library;
tools/build_dbg.sh builds another one).  Inputs are np.random.default_rng streams with fixed seeds;
nothing outside the repository is read.
usage: python tools/pass_digest.py"""
import functools
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtsdr as sdr  # noqa: E402

CTX = sdr.get_context()
NS = (1, 2, 7, 4095, 4096, 4097, 3 * 4096 + 5, 2048 * 4096 + 25)     # the last: more than 2048 minimum chunks
GUARD = 8                                                           # floats behind the output


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


@functools.lru_cache(maxsize=4)
def capture(n, fmt, seed):
    """n complex samples of interleaved IQ in the format's type"""
    rng = np.random.default_rng(seed)
    if fmt == "cf32":
        return (0.4 * rng.standard_normal(2 * n, dtype=np.float32) + np.float32(0.05)).astype(np.float32)
    if fmt == "cu8":
        return rng.integers(0, 256, 2 * n, dtype=np.uint8)
    if fmt == "cs8":
        return rng.integers(-128, 128, 2 * n, dtype=np.int8)
    return rng.integers(-2048, 2048, 2 * n, dtype=np.int16)           # a 12-bit ADC's codes, rails included


def placements(es, in_place):
    """(input offset, output offset) in bytes past a 16-B boundary; None: out == in"""
    ins = (0, es) + ((2, 6) if es == 2 else ())
    outs = (0, 8)
    p = [(i, o) for i in dict.fromkeys(ins) for o in outs]
    if in_place:
        p += [(0, None), (8, None)]
    return p


def run_capture_pass(tag, fmt, n, in_off, out_off, call, state):
    """one placement of one block: the calls of `call` on it, a line each"""
    x = capture(n, fmt, 1000 + n % 997)
    din = sdr.DeviceBuffer(CTX, x.nbytes + 32)
    assert din.ptr % 16 == 0
    din.upload(x, in_off)
    if out_off is None:
        dout, optr, whole = din, din.ptr + in_off, (x.nbytes + 32) // 4
    else:
        whole = 2 * n + GUARD + 4
        dout = sdr.DeviceBuffer(CTX, 4 * whole)
        dout.zero()
        optr = dout.ptr + out_off
    for k, arg in enumerate(call):
        if out_off is None and k:
            din.upload(x, in_off)                                   # in place: the block again
        arg(din.ptr + in_off, n, optr)
        print(f"{tag} n={n} in+{in_off} out{'=in' if out_off is None else '+' + str(out_off)} call {k} "
              f"{sha(dout.download(whole, dtype=np.uint32))} {state()}")
    if dout is not din:
        dout.free()
    din.free()


def some(n, places):
    """every placement at the small sizes, the first and the last at the large one"""
    return places if n < 1 << 20 else (places[0], places[-1])


def iqc():
    for dt, fmt in ((np.float32, "cf32"), (np.uint8, "cu8")):
        es = 8 if fmt == "cf32" else 2
        for n in NS:
            for in_off, out_off in some(n, placements(es, fmt == "cf32")):
                c = sdr.IqCorrector(dt, ctx=CTX)
                calls = [lambda i, m, o, e=e: c.process_dev(i, m, o, estimate=e) for e in (True, False, True)]
                run_capture_pass(f"iqc_{fmt}", fmt, n, in_off, out_off, calls, lambda: sha(c.raw_state()))
                c.close()


def ingest():
    for fmt, bits in (("cf32", None), ("cu8", None), ("cs8", None), ("cs16", 12)):
        es = 2 * sdr.capture.FORMATS[fmt][0].itemsize
        for swap, meter in ((False, True), (True, True), (False, False)):
            for n in NS:
                places = some(n, placements(es, fmt == "cf32")) if meter and not swap else [(es, 8)]
                for in_off, out_off in places:
                    g = sdr.CaptureIngest(fmt, bits=bits, swap=swap, meter=meter, ctx=CTX)
                    run_capture_pass(f"ingest_{fmt}{'_swap' if swap else ''}{'' if meter else '_bare'}", fmt, n, in_off, out_off,
                                     [g.process_dev], lambda: sha(repr(tuple(g.meter())).encode()))
                    g.close()


def rmeter():
    rows = 3
    for W in (64, 100, 4095, 4096, 16385, 40000):                      # both kernels; 1, 2 and 3 slots a window
        calls = (1, 63, W - 1, W, 3 * W + 17, 70000)
        for off in (0, 4):
            m = sdr.RowMeter(rows, W, nbins=64, scale=np.float32(20.0), limit=np.float32(1.0), ctx=CTX)
            for k, n in enumerate(calls):
                x = np.random.default_rng(7000 + W + k).standard_normal((rows, n + 3), dtype=np.float32)
                if n > 40:
                    x[1, 17], x[1, 40] = np.nan, np.inf                 # one row with a NaN and an infinity
                buf = sdr.DeviceBuffer(CTX, x.nbytes + 16)
                buf.upload(x, off)
                m.process_dev(buf.ptr + off, n + 3, n)
                r = m.records()
                print(f"rmeter W={W} row+{off} call {k} n={n} {sha(*r)} {sha(m.hist())} {sha(m.windows())}")
                buf.free()
            m.close()


iqc()
ingest()
rmeter()
