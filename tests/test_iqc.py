"""The device-side IQ imbalance / DC offset corrector (IqCorrector, csrc/iqc.hip) against the host
model rtsdr.IqBalance (tests/test_iqc_model.py pins that on the CPU), float32 and uint8.

What is compared, after every call:
  moments       uint8: the five smoothed moments equal the model's exactly (integer sums, then the
                model's own operations).  float32: each block moment is within 2^-53 sum|terms| of
                math.fsum(terms) / n -- n 2^-53 sum|terms| on the sum, the a-priori bound of any
                summation order, so it does not constrain the kernel's tree.
  coefficients  the model's step 3 on the device's own downloaded moments, to within 4 f64 ulps
                (slack for a contracted multiply-add; the kernel is built without contraction).
  rows          within one float32 ulp of the model's step 4 with the device's coefficients; the
                share of values that differ at all is printed, not bounded.
The input sits between guards a stray read would show in the moments (1e30 / byte 255), the output
between guards of a float pattern that must come back untouched."""
import ctypes
import math

import numpy as np
import pytest
from scipy.signal import firwin, lfilter

import iqc_capture as cap

pytestmark = pytest.mark.gpu

CHUNK = 4096         # samples of a workgroup's chunk in the moments pass (include/sdr.h SDR_IQC_CHUNK, IqCorrector.CHUNK)
RAGGED = 2 * CHUNK + 4095                      # three chunks, the last one a sample short and odd
SHAPES = (1, 2, 63, 64, 65, 4097, 32771, RAGGED)
NMAX = max(SHAPES)
GUARD = 64                                     # floats on either side of out
SENTINEL = np.float32(-7.25e12)
DTYPES = (np.float32, np.uint8)
U53 = 2.0 ** -53


def _layouts(dtype):
    """(iq offset from a 16-byte boundary in complex samples, out offset in floats): every head of
    both passes, and out in and out of phase with the pairs"""
    ins = (0, 1, 3) if dtype == np.uint8 else (0, 1)
    return [(i, o) for i in ins for o in (0, 2)]


class Bench:
    """One input and one output allocation, reused by the calls of a test."""

    def __init__(self, sdr, ctx, dtype, nmax):
        self.sdr, self.ctx, self.u8 = sdr, ctx, np.dtype(dtype) == np.uint8
        self.es = 2 if self.u8 else 8
        self.bin = sdr.DeviceBuffer(ctx, self.es * (nmax + 16) + 64)
        self.bout = sdr.DeviceBuffer(ctx, 4 * (2 * nmax + 2 * GUARD + 8))
        assert self.bin.ptr % 256 == 0 and self.bout.ptr % 256 == 0

    def call(self, corr, x, in_off=0, out_off=0, estimate=True):
        n = len(x) // 2
        fill = 255 if self.u8 else 1e30
        host = np.full(2 * (n + 16), fill, dtype=x.dtype)
        host[2 * (8 + in_off):2 * (8 + in_off + n)] = x           # 8 samples = 16 B (u8) or 64 B (f32) of guard in front
        self.bin.upload(host)
        iq_ptr = self.bin.ptr + self.es * (8 + in_off)
        assert (iq_ptr - self.es * in_off) % 16 == 0
        self.bout.upload(np.full(2 * n + 2 * GUARD + out_off, SENTINEL, dtype=np.float32))
        out_ptr = self.bout.ptr + 4 * (GUARD + out_off)
        corr.process_dev(iq_ptr, n, out_ptr, estimate)
        got = self.bout.download(2 * n + 2 * GUARD + out_off)
        lo, hi = got[:GUARD + out_off], got[GUARD + out_off + 2 * n:]
        assert np.all(lo == SENTINEL) and np.all(hi == SENTINEL) and len(hi) == GUARD, "a store outside out"
        return got[GUARD + out_off:GUARD + out_off + 2 * n].copy()

    def free(self):
        self.bin.free()
        self.bout.free()


def _pairs(x):
    v = np.asarray(x).astype(np.float64)
    if np.asarray(x).dtype == np.uint8:
        v = (v - 128.0) / 128.0
    return v[0::2], v[1::2]


def _terms(x):
    i, q = _pairs(x)
    return i, q, i * i, q * q, i * q


def _ulps64(a, b):
    a, b = np.float64(a), np.float64(b)
    return 0.0 if a == b else float(abs(a - b) / np.spacing(max(abs(a), abs(b))))


def _check_coefficients(sdr, st, dc=True, balance=True, prev=None):
    """the device's coefficients against the model's step 3 on the device's own moments"""
    from importlib import import_module
    iqb = import_module(sdr.IqBalance.__module__)
    want = iqb.coefficients(st[:5], dc, balance)
    if want is None:
        want = prev
    worst = max(_ulps64(g, w) for g, w in zip(st[5:9], want))
    assert worst <= 4.0, (st[5:9], want, worst)
    return worst


def _check_rows(sdr, y, x, coeff, what=""):
    """within one float32 ulp of the model's step 4 with the coefficients the device used"""
    from importlib import import_module
    iqb = import_module(sdr.IqBalance.__module__)
    ref = iqb.apply(*_pairs(x), coeff)
    assert y.shape == ref.shape and np.array_equal(np.isnan(y), np.isnan(ref))
    ok = ~np.isnan(ref)
    err = np.abs(y[ok].astype(np.float64) - ref[ok].astype(np.float64))
    differ = float(np.mean(y[ok] != ref[ok])) if np.any(ok) else 0.0
    assert np.all(err <= np.spacing(np.abs(ref[ok])).astype(np.float64)), what
    return differ


@pytest.mark.parametrize("dtype", DTYPES)
def test_shapes_and_alignments(sdr, gpu_ctx, dtype):
    """one call per shape and layout from the initial state: moments, coefficients, rows, guards"""
    assert CHUNK == sdr.IqCorrector.CHUNK
    full = cap.capture(NMAX, dtype)
    b = Bench(sdr, gpu_ctx, dtype, NMAX)
    corr = sdr.IqCorrector(dtype, ctx=gpu_ctx)
    worst_c, worst_m, differ = 0.0, 0.0, 0.0
    try:
        for n in SHAPES:
            x = full[2 * (NMAX - n):]                             # the tail: another slice per n
            terms = _terms(x)
            model = sdr.IqBalance(dtype)
            ym = model.process(x)
            ms = model.state()
            for in_off, out_off in _layouts(dtype):
                corr.reset()
                y = b.call(corr, x, in_off, out_off)
                st = corr.state()
                assert (st.updates, st.skipped, st.holds) == (ms.updates, ms.skipped, ms.holds) == (1, 0, ms.holds), (n, in_off)
                if dtype == np.uint8:
                    assert st[:5] == ms[:5], (n, in_off, out_off)
                else:
                    for k in range(5):
                        bound = U53 * float(np.sum(np.abs(terms[k])))
                        err = abs(st[k] - math.fsum(terms[k]) / n)
                        worst_m = max(worst_m, err / bound if bound else 0.0)
                        assert err <= bound, (n, in_off, k, err, bound)
                worst_c = max(worst_c, _check_coefficients(sdr, st, prev=(0.0, 0.0, 0.0, 1.0)))
                differ = max(differ, _check_rows(sdr, y, x, st[5:9], (n, in_off, out_off)))
                if dtype == np.uint8:                             # the same moments: the same rows as the model to an ulp
                    assert np.all(np.abs(y.astype(np.float64) - ym) <= np.spacing(np.abs(ym)))
    finally:
        corr.close()
        b.free()
    print(f"iqc {np.dtype(dtype).name}: coefficients within {worst_c:.1f} ulps, f32 moments at most {worst_m:.2e} of the bound, "
          f"at most {100 * differ:.3f} % of a call's values differ from the model's rounding")


@pytest.mark.parametrize("dtype", DTYPES)
def test_sequence_and_reset(sdr, gpu_ctx, dtype):
    """four calls of different n with the state carried, against the model carried across them; the
    same sequence after reset() gives the same bits"""
    lens = (4097, CHUNK + 3, 65, 20001)
    x = cap.capture(sum(lens), dtype, seed=1)
    b = Bench(sdr, gpu_ctx, dtype, max(lens))
    corr = sdr.IqCorrector(dtype, rate=0.25, ctx=gpu_ctx)
    runs = []
    try:
        for rep in range(2):
            if rep:
                corr.reset()
            model = sdr.IqBalance(dtype, rate=0.25)
            o, res, top = 0, [], 0.0
            for k, n in enumerate(lens):
                blk = x[2 * o:2 * (o + n)]
                o += n
                y = b.call(corr, blk, in_off=k % 2, out_off=2 * (k // 2 % 2))
                st = corr.state()
                model.process(blk)
                ms = model.state()
                assert (st.updates, st.skipped, st.holds) == (k + 1, 0, 0) == (ms.updates, ms.skipped, ms.holds)
                if dtype == np.uint8:
                    assert st[:5] == ms[:5], k
                else:
                    # a block moment of either side is within 2^-53 sum|terms| of the exact mean; the
                    # smoothed ones are convex combinations of them, plus a few roundings of the smoothing
                    top = max(top, max(float(np.sum(np.abs(t))) for t in _terms(blk)))
                    for g, w in zip(st[:5], ms[:5]):
                        assert abs(g - w) <= 2 * U53 * top + 16 * np.spacing(abs(w)), (k, g, w)
                _check_coefficients(sdr, st)
                _check_rows(sdr, y, blk, st[5:9], k)
                res.append((y, corr.raw_state()))
            runs.append(res)
        for (y0, s0), (y1, s1) in zip(*runs):
            assert np.array_equal(y0, y1) and np.array_equal(s0, s1)
    finally:
        corr.close()
        b.free()


def test_in_place_equals_out_of_place(sdr, gpu_ctx):
    n = CHUNK + 4097
    x = cap.capture(n, np.float32, seed=2)
    b = Bench(sdr, gpu_ctx, np.float32, n)
    c0, c1 = sdr.IqCorrector(ctx=gpu_ctx), sdr.IqCorrector(ctx=gpu_ctx)
    try:
        for off in (0, 1):                                        # 16-B aligned, and one complex sample past it
            c0.reset()
            c1.reset()
            y = b.call(c0, x, in_off=off, out_off=2 * off)
            host = np.full(2 * (n + 16), 1e30, dtype=np.float32)
            host[2 * (8 + off):2 * (8 + off + n)] = x
            b.bin.upload(host)
            ptr = b.bin.ptr + 8 * (8 + off)
            c1.process_dev(ptr, n, ptr)
            got = b.bin.download(2 * (n + 16))
            assert np.array_equal(got[2 * (8 + off):2 * (8 + off + n)], y)
            assert np.all(got[:2 * (8 + off)] == np.float32(1e30)) and np.all(got[2 * (8 + off + n):] == np.float32(1e30))
            assert np.array_equal(c0.raw_state(), c1.raw_state())
    finally:
        c0.close()
        c1.close()
        b.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_estimate_off_applies_the_installed_coefficients(sdr, gpu_ctx, dtype):
    n = 4099
    x = cap.capture(n, dtype)
    b = Bench(sdr, gpu_ctx, dtype, n)
    corr = sdr.IqCorrector(dtype, ctx=gpu_ctx)
    try:
        y = b.call(corr, x, estimate=False)                       # the initial state: the identity
        i, q = _pairs(x)
        assert np.array_equal(y[0::2], i.astype(np.float32)) and np.array_equal(y[1::2], q.astype(np.float32))
        installed = (0.03, -0.02, cap.C1, cap.C2)
        corr.set(*installed)
        y = b.call(corr, x, in_off=1, estimate=False)
        st = corr.state()
        assert st[5:9] == installed and (st.updates, st.skipped, st.holds) == (0, 0, 0) and st[:5] == (0.0,) * 5
        _check_rows(sdr, y, x, installed)
        assert cap.image_db(x, 3.1e6) - cap.image_db(y, 3.1e6) >= 20.0
        got = np.empty(4)
        p = corr.coeffs_ptr
        sdr._lib.check(gpu_ctx.lib.sdr_memcpy_d2h(gpu_ctx.handle, got.ctypes.data, p, 32), "d2h")
        assert tuple(got) == installed
        b.call(corr, x)                                           # an estimate replaces them
        assert corr.state().updates == 1 and corr.state()[5:9] != installed
    finally:
        corr.close()
        b.free()


def test_nan_block(sdr, gpu_ctx):
    """a NaN in the second block: the same skipped count, coefficients and rows as the model"""
    n = 8192
    x = np.array(cap.capture(2 * n, np.float32, seed=1))
    x[2 * (n + 100)] = np.nan
    x[2 * (n + 7000) + 1] = np.nan
    b = Bench(sdr, gpu_ctx, np.float32, n)
    corr, model = sdr.IqCorrector(ctx=gpu_ctx), sdr.IqBalance()
    try:
        b.call(corr, x[:2 * n])
        model.process(x[:2 * n])
        before = corr.state()
        y = b.call(corr, x[2 * n:], in_off=1)
        model.process(x[2 * n:])
        st, ms = corr.state(), model.state()
        assert (st.updates, st.skipped, st.holds) == (ms.updates, ms.skipped, ms.holds) == (1, 1, 0)
        assert st[:9] == before[:9]
        _check_rows(sdr, y, x[2 * n:], st[5:9])
        assert list(np.flatnonzero(np.isnan(y))) == [200, 201, 14001]
    finally:
        corr.close()
        b.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_flags_holds_and_run(sdr, gpu_ctx, dtype):
    """dc / balance off, a hold, and the synchronous host call"""
    n = 8192
    x = cap.capture(n, dtype)
    for kw in (dict(dc=False), dict(balance=False), dict(rate=1.0)):
        corr, model = sdr.IqCorrector(dtype, ctx=gpu_ctx, **kw), sdr.IqBalance(dtype, **kw)
        try:
            y, ym = corr.run(x), model.process(x)
            st, ms = corr.state(), model.state()
            _check_coefficients(sdr, st, kw.get("dc", True), kw.get("balance", True))
            _check_rows(sdr, y, x, st[5:9])
            if dtype == np.uint8:
                assert st[:5] == ms[:5]
            assert np.allclose(y, ym, rtol=0, atol=1e-6)
            if "dc" in kw:
                assert (st.dI, st.dQ) == (0.0, 0.0)
            if "balance" in kw:
                assert (st.c1, st.c2) == (0.0, 1.0)
            # an all-zero block, a constant block and Q = I as the first update after a reset: the
            # installed coefficients stay and holds counts
            if dtype == np.uint8:
                holds = (np.full(1554, 128, np.uint8), np.tile(np.array([200, 56], np.uint8), 777), np.repeat(np.arange(777, dtype=np.uint8), 2))
            else:
                holds = (np.zeros(1554, np.float32), np.tile(np.array([0.25, -0.5], np.float32), 777),
                         np.repeat((np.arange(777) / 1024.0 - 0.375).astype(np.float32), 2))
            for blk in holds:
                corr.reset()
                corr.set(*st[5:9])
                y = corr.run(blk)
                s2 = corr.state()
                assert s2[5:9] == st[5:9] and (s2.updates, s2.skipped, s2.holds) == (1, 0, 1)
                _check_rows(sdr, y, blk, s2[5:9])
        finally:
            corr.close()


def test_into_the_filter_bank(sdr, gpu_ctx):
    """IqCorrector.process_dev -> FilterBank.process_dev on the corrected buffer, against the f64
    filter bank definition on the model-corrected capture, within tests/test_pfb.py's bound
    1e-6 |y| + 5e-7 sum|h| max|x|"""
    M, D, T, n = 8, 4, 64, 4096
    h = firwin(T, 1.0 / M)
    x = cap.capture(n, np.float32)
    ym = sdr.IqBalance().process(x).astype(np.float64)
    z = ym[0::2] + 1j * ym[1::2]
    km = np.arange(n) % M
    ref = np.stack([lfilter(h, 1.0, z * np.exp(-2j * np.pi * ((c * km) % M) / M))[::D] for c in range(M)])
    G = float(np.sum(np.abs(h)) * np.max(np.abs(z)))
    corr = sdr.IqCorrector(ctx=gpu_ctx)
    fb = sdr.FilterBank(M, cap.FS, D, taps=h, ctx=gpu_ctx)
    bin_, mid, rows = sdr.DeviceBuffer.from_array(gpu_ctx, x), sdr.DeviceBuffer(gpu_ctx, 8 * n), sdr.DeviceBuffer(gpu_ctx, 8 * M * (n // D))
    try:
        corr.process_dev(bin_.ptr, n, mid.ptr)
        fb.process_dev(mid.ptr, n, rows.ptr, n // D)
        y = rows.download(2 * M * (n // D)).view(np.complex64).reshape(M, n // D)
        err = np.abs(y.astype(np.complex128) - ref)
        worst = float(np.max(err / (1e-6 * np.abs(ref) + 5e-7 * G)))
        print(f"iqc -> pfb: max err {np.max(err):.3e}, {worst:.3f} of the bound")
        assert worst <= 1.0
        # bin 7 (centred on -2.4 MHz) holds no station, only the image of the one at +3.1 MHz: the
        # bank on the uncorrected capture holds 20 dB more there
        fb.reset()
        fb.process_dev(bin_.ptr, n, rows.ptr, n // D)
        raw = rows.download(2 * M * (n // D)).view(np.complex64).reshape(M, n // D)
        ratio = float(np.mean(np.abs(raw[7]) ** 2) / np.mean(np.abs(y[7]) ** 2))
        print(f"bin 7: {10 * np.log10(ratio):.1f} dB less after the correction")
        assert ratio >= 100.0
    finally:
        fb.close()
        corr.close()
        for d in (bin_, mid, rows):
            d.free()


def test_c_entry_point_refuses_bad_calls(sdr, gpu_ctx):
    """SDR_EINVAL from the C side with a live object, before any launch: the state stays initial"""
    lib = gpu_ctx.lib
    buf = sdr.DeviceBuffer(gpu_ctx, 1 << 16)
    cf, c8 = sdr.IqCorrector(ctx=gpu_ctx), sdr.IqCorrector(np.uint8, ctx=gpu_ctx)
    try:
        hf, h8, p = cf._open(), c8._open(), buf.ptr
        for h, args, word in ((hf, (p, 0, p + 32768, 1), "n="), (hf, (p, 2 ** 31, p + 32768, 1), "n="), (hf, (None, 8, p, 1), "NULL"),
                              (hf, (p, 8, None, 1), "NULL"), (hf, (p + 4, 8, p + 32768, 1), "aligned"), (hf, (p, 8, p + 32772, 1), "aligned"),
                              (h8, (p + 1, 8, p + 32768, 1), "aligned"), (hf, (p, 8, p + 8, 1), "overlap"), (hf, (p + 8, 8, p, 1), "overlap"),
                              (h8, (p, 8, p, 1), "overlap"), (h8, (p + 60, 8, p, 1), "overlap")):
            assert lib.sdr_iqc_process_dev(h, *args) == -1 and word in lib.sdr_last_error().decode(), (args, lib.sdr_last_error())
        bad = (ctypes.c_double * 4)(0.0, 0.0, float("nan"), 1.0)
        assert lib.sdr_iqc_set(hf, bad) == -1 and "finite" in lib.sdr_last_error().decode()
        assert cf.state()[:12] == (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0, 0, 0)
    finally:
        cf.close()
        c8.close()
        buf.free()
