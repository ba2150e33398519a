"""The wideband spectrum / waterfall (sdr_spec, csrc/spectrum.hip; rtsdr.Spectrum) and the station
finder (rtsdr.find_channels).  Parity is against the f64 definition
    X_s[k]    = sum_{i < nfft} w[i] x[s hop + i] exp(-2 pi i k i / nfft)
    out[r][j] = (1 / (navg (sum w)^2)) sum_{s in row r} |X_s[k]|^2,   k = (j + nfft / 2) mod nfft
which test_reference_form pins to scipy.signal.spectrogram.

Tolerance: the channelizer's and the filter bank's (tests/test_ddc.py, tests/test_pfb.py), carried
over to the amplitude X_s[k] -- the same object as their sum_j h[j] x[...] e^{...} with h -> w.
With G = sum|w| max(|re x|, |im x|) and d_s[k] = 1e-6 |X_s[k]| + 5e-7 G,
    |out - ref|[r][j] <= mean_s(2 |X_s[k]| d_s[k] + d_s[k]^2) / (sum w)^2.
test_tolerance_is_reachable_in_f32 shows without a GPU that an f32 FFT stays under a quarter of
it.  The GPU tests print the share of the bound they use."""
import ctypes

import numpy as np
import pytest
import scipy.fft
from scipy.signal import get_window, spectrogram

SPLIT_SEGS = 8       # the implementation's split threshold (include/sdr.h SDR_SPEC_SPLIT_SEGS): a row of more segments may be summed in chunks
TARGET_CHUNKS = 2048  # csrc/spectrum.hip SPEC_TARGET_CHUNKS: the chunks grow beyond SPLIT_SEGS once a call has more than 8 x 2048 segments
SIZES = (64, 128, 256, 512, 1024, 2048, 4096, 8192)


# ---- the f64 reference ----------------------------------------------------------------------
def to_complex(iq, u8=False):
    v = (iq.astype(np.float64) - 128.0) / 128.0 if u8 else iq.astype(np.float64)
    return v[0::2] + 1j * v[1::2]


def interleave(z):
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=1).reshape(-1), dtype=np.float32)


def geometry(n, nfft, hop, navg):
    nseg = (n - nfft) // hop + 1
    na = navg if navg > 0 else nseg
    return nseg, na, nseg // na


def ref_segments(z, nfft, hop, navg, w):
    """X_s[k], shifted to ascending frequency, of the segments that fill rows: complex128
    [rows, navg, nfft]"""
    nseg, na, rows = geometry(len(z), nfft, hop, navg)
    seg = np.lib.stride_tricks.sliding_window_view(z, nfft)[::hop][:rows * na]
    X = scipy.fft.fft(seg * w, axis=-1)
    return np.fft.fftshift(X, axes=-1).reshape(rows, na, nfft)


def ref_spectrum(z, nfft, hop, navg, w):
    """(rows of power, their tolerance, the rows' mean amplitude tolerance d in units of G), f64"""
    X = np.abs(ref_segments(z, nfft, hop, navg, w))
    G = float(np.sum(np.abs(w)) * max(np.max(np.abs(z.real)), np.max(np.abs(z.imag))))
    d = 1e-6 * X + 5e-7 * G
    s2 = float(np.sum(w)) ** 2
    return np.mean(X * X, axis=1) / s2, np.mean(2.0 * X * d + d * d, axis=1) / s2, np.mean(d, axis=1) / G


def check(y, ref, bound, what="", dg=None):
    """dg: prints the share of the bound as an amplitude error too -- to first order the bound is
    2 |X| d, so a share s of it is an amplitude error of s d"""
    share = np.abs(y.astype(np.float64) - ref) / bound
    worst = float(np.max(share))
    amp = f" = {float(np.max(share * dg)):.2e} G in amplitude" if dg is not None else ""
    print(f"spectrum {what}: {worst:.4f} of the bound{amp}")
    assert y.shape == ref.shape and y.dtype == np.float32
    assert worst <= 1.0, (what, worst)
    return worst


def noise_iq(n, seed, u8=False):
    rng = np.random.default_rng(seed)
    if u8:
        return rng.integers(0, 256, 2 * n, dtype=np.uint8)
    return (0.5 * rng.standard_normal(2 * n)).astype(np.float32)


def tones_iq(n, M, u8=False):
    """tests/test_pfb.py tones_iq -- three tones at full scale: on a bin, between two bins, near
    the band edge (scaled by 1 / 2 and quantised for a u8 capture)"""
    k = np.arange(n)
    z = sum(a * np.exp(2j * np.pi * (nu * k + 0.1 * i)) for i, (a, nu) in enumerate(zip((1.0, 0.3, 0.5), (1.0 / M, 0.123456, -0.31))))
    if u8:
        return np.clip(np.rint(128.0 + 64.0 * interleave(z).astype(np.float64)), 0, 255).astype(np.uint8)
    return interleave(z)


def window_of(name, nfft):
    return get_window(name, nfft).astype(np.float64)


# ---- the synthetic FM band --------------------------------------------------------------------
BAND_FS, BAND_BINS, BAND_NFFT, BAND_N = 19.2e6, 96, 4096, 1 << 18
PLANTED = ((-31, 0.5), (2, 0.05), (17, 0.02))
WEAK = (-30, 0.5 * 10 ** (-25 / 20))          # 25 dB below the strongest, in the slot next to it

_band = {}


def band_iq(sdr, weak=False):
    """three FM stations (synth.fm_iq at 19.2 MS/s) mixed to bins -31, 2 and 17 of 96 with
    amplitudes 0.5, 0.05, 0.02, plus noise; weak: a fourth, 25 dB below the strongest, next to it"""
    if weak not in _band:
        k = np.arange(BAND_N)
        z = np.zeros(BAND_N, np.complex128)
        for i, (b, a) in enumerate(PLANTED + ((WEAK,) if weak else ())):
            s = to_complex(sdr.synth.fm_iq(BAND_N, seed=10 + i, fs=BAND_FS, snr_db=60.0))
            z += a * s * np.exp(2j * np.pi * ((b * k) % BAND_BINS) / BAND_BINS)
        rng = np.random.default_rng(99)
        z += 2e-3 * (rng.standard_normal(BAND_N) + 1j * rng.standard_normal(BAND_N))
        _band[weak] = z
    return _band[weak]


def band_row(z):
    return ref_spectrum(z, BAND_NFFT, BAND_NFFT, 0, window_of("hann", BAND_NFFT))[0][0]


# ---- CPU ------------------------------------------------------------------------------------
@pytest.mark.parametrize("navg", (1, 3, 0))
@pytest.mark.parametrize("hop", (256, 128, 129))
def test_reference_form(sdr, hop, navg):
    """the reference helper is scipy.signal.spectrogram(..., scaling='spectrum', mode='psd')
    averaged over groups of navg columns and shifted; freqs_hz is its shifted frequency axis"""
    nfft, fs, n = 256, 1.0e6, 256 * 11 + 77
    z = to_complex(noise_iq(n, 1))
    for name in ("hann", "boxcar", "flattop"):
        w = window_of(name, nfft)
        f, _, S = spectrogram(z, fs=fs, window=w, nperseg=nfft, noverlap=nfft - hop, detrend=False, return_onesided=False,
                              scaling="spectrum", mode="psd")
        nseg, na, rows = geometry(n, nfft, hop, navg)
        assert S.shape == (nfft, nseg)
        want = np.fft.fftshift(S, axes=0).T[:rows * na].reshape(rows, na, nfft).mean(axis=1)
        got = ref_spectrum(z, nfft, hop, navg, w)[0]
        assert got.shape == (rows, nfft) and np.allclose(got, want, rtol=1e-10, atol=1e-18)
        sp = sdr.Spectrum(nfft, fs, hop=hop, navg=navg, window=name)
        assert np.allclose(sp.freqs_hz, np.fft.fftshift(f)) and np.all(np.diff(sp.freqs_hz) > 0)
        assert np.array_equal(sp.window, w) and sp.scale == float(np.sum(w)) ** 2
        assert sp.rows(n) == (nseg, rows)


def test_reference_form_sparse(sdr):
    """hop > nfft: explicit slicing"""
    nfft, hop, n = 64, 64 + 37, 64 * 20
    z = to_complex(noise_iq(n, 2))
    w = window_of("hann", nfft)
    nseg, na, rows = geometry(n, nfft, hop, 2)
    assert sdr.Spectrum(nfft, 1.0, hop=hop, navg=2).rows(n) == (nseg, rows)
    got = ref_spectrum(z, nfft, hop, 2, w)[0]
    P = [np.abs(np.fft.fftshift(np.fft.fft(w * z[s * hop:s * hop + nfft]))) ** 2 / np.sum(w) ** 2 for s in range(nseg)]
    want = np.array([(P[2 * r] + P[2 * r + 1]) / 2 for r in range(rows)])
    assert rows == nseg // 2 and np.allclose(got, want, rtol=1e-12, atol=0)


def test_rows(sdr):
    S = sdr.Spectrum
    assert S(64, 1.0).rows(64) == (1, 1)
    assert S(64, 1.0, hop=10).rows(64 + 9) == (1, 1) and S(64, 1.0, hop=10).rows(64 + 10) == (2, 1)
    assert S(64, 1.0, hop=10, navg=1).rows(64 + 10) == (2, 2)
    assert S(64, 1.0, hop=64, navg=3).rows(64 * 11 + 5) == (11, 3)          # two segments left over
    assert S(64, 1.0, hop=100, navg=0).rows(64 + 100 * 6) == (7, 1)
    assert S(4096, 1.0, hop=1 << 24, navg=1).rows((1 << 28) + 4096) == (17, 17)
    assert sdr.spectrum_rows(1 << 30, 64, 1, 0) == ((1 << 30) - 63, 1)
    for n, kw in ((63, {}), (64 * 2, dict(navg=3))):
        with pytest.raises(ValueError):
            S(64, 1.0, **kw).rows(n)


def test_argument_errors_before_device_work(sdr):
    """Python raises ValueError before a context exists; the C entry point refuses the same
    arguments (SDR_EINVAL with a message naming the argument) before it looks at its context."""
    S = sdr.Spectrum
    w = np.ones(64)
    for kw in (dict(nfft=32), dict(nfft=16384), dict(nfft=96), dict(hop=0), dict(hop=(1 << 24) + 1), dict(navg=-1),
               dict(window=np.r_[w[:-1], np.nan]), dict(window=np.r_[w[:32], -w[:32]]), dict(window=w[:63]),
               dict(iq_dtype=np.int16), dict(fs=0.0)):
        with pytest.raises(ValueError):
            S(**dict(dict(nfft=64, fs=1.0), **kw))
    sp = S(64, 1.0, navg=3)
    for n in (63, 64 * 2):                                   # n < nfft; no complete row
        with pytest.raises(ValueError):
            sp.process_dev(16, n, 16)
        with pytest.raises(ValueError):
            sp.run(np.zeros(2 * n, np.float32))
    with pytest.raises(ValueError):
        sp.process_dev(16, 64 * 3, 16, out_stride=63)
    assert sp.handle is None                                 # nothing touched a device
    lib = sdr.load_library()
    dp = ctypes.POINTER(ctypes.c_double)
    out = ctypes.c_void_p()

    def create(nfft, window, hop, navg, dtype=0):
        wp = None if window is None else np.asarray(window, dtype=np.float64).ctypes.data_as(dp)
        return lib.sdr_spec_create(None, nfft, wp, hop, navg, dtype, ctypes.byref(out))
    for args, word in (((32, None, 32, 1), "nfft"), ((16384, None, 64, 1), "nfft"), ((96, None, 64, 1), "nfft"),
                       ((64, None, 0, 1), "hop"), ((64, None, (1 << 24) + 1, 1), "hop"), ((64, None, 64, -1), "navg"),
                       ((64, np.r_[w[:-1], np.inf], 64, 1), "window[63]"), ((64, np.r_[w[:32], -w[:32]], 64, 1), "window sums"),
                       ((64, None, 64, 1, 2), "dtype"), ((64, None, 64, 1), "context is NULL"), ((64, w, 1, 0, 1), "context is NULL")):
        assert create(*args) == -1 and word in lib.sdr_last_error().decode(), (args, lib.sdr_last_error())
    assert lib.sdr_spec_create(None, 64, None, 64, 1, 0, None) == -1 and "out" in lib.sdr_last_error().decode()
    assert lib.sdr_spec_process_dev(None, None, 64, None, 64) == -1 and "NULL" in lib.sdr_last_error().decode()
    assert lib.sdr_spec_run(None, None, 64, None, 64) == -1 and "NULL" in lib.sdr_last_error().decode()
    assert lib.sdr_spec_rows(None, 64, None, None) == -1 and "NULL" in lib.sdr_last_error().decode()


def tone_cases(nfft):
    k = np.arange(6 * nfft)
    return {"noise": to_complex(noise_iq(6 * nfft, 3)), "u8 noise": to_complex(noise_iq(6 * nfft, 4, u8=True), u8=True),
            "tones": to_complex(tones_iq(6 * nfft, nfft)),
            # full scale on a bin, 1e-7 of it elsewhere: beyond 140 dB between the largest and the smallest bin
            "deep": np.exp(2j * np.pi * 5 * k / nfft) + 1e-7 * np.exp(2j * np.pi * 0.3 * k)}


def test_tolerance_is_reachable_in_f32(sdr):
    """a complex64 FFT of the windowed segments (f32 window, f32 product) against the f64
    reference: under a quarter of the bound, so f32 arithmetic can meet it with a margin of four"""
    worst = 0.0
    for nfft in (64, 256, 4096, 8192):
        for name in ("hann", "boxcar"):
            w = sdr.design.spectrum_window(name, nfft)               # the windows Spectrum uses
            assert np.array_equal(w, window_of(name, nfft))
            for what, z in tone_cases(nfft).items():
                z = z.astype(np.complex64).astype(np.complex128)     # the capture is f32: both sides see the same samples
                ref, bound, _ = ref_spectrum(z, nfft, nfft, 0, w)
                seg = z.astype(np.complex64).reshape(-1, nfft) * w.astype(np.float32)
                X = np.fft.fftshift(scipy.fft.fft(seg.astype(np.complex64), axis=-1), axes=-1)
                assert X.dtype == np.complex64
                P = np.mean(np.abs(X.astype(np.complex128)) ** 2, axis=0) / np.sum(w) ** 2
                share = float(np.max(np.abs(P - ref[0]) / bound[0]))
                worst = max(worst, share)
                if what == "deep":
                    assert np.max(ref) / np.min(ref) > 1e14          # > 140 dB in power
    print(f"f32 FFT: {worst:.4f} of the bound")
    assert worst < 0.25


def test_find_channels(sdr):
    fc = sdr.find_channels
    row = band_row(band_iq(sdr))
    found = fc(row, BAND_FS, BAND_FS / BAND_BINS)
    assert list(found.index) == [-31, 2, 17] and found.index.dtype == np.int64
    assert np.allclose(found.freq_hz, np.array([-31, 2, 17]) * 200e3) and np.all(found.snr_db >= 10.0)
    assert np.all(np.diff(found.snr_db) < 0)                 # amplitudes 0.5, 0.05, 0.02
    # the station next to the strongest: never with isolated=True; without it, with the
    # strongest one's skirts, whenever it is over the threshold
    roww = band_row(band_iq(sdr, weak=True))
    assert list(fc(roww, BAND_FS, BAND_FS / BAND_BINS).index) == [-31, 2, 17]
    loose = fc(roww, BAND_FS, BAND_FS / BAND_BINS, isolated=False)
    assert {-31, -30, 2, 17} <= set(loose.index)
    allc = fc(roww, BAND_FS, BAND_FS / BAND_BINS, min_snr_db=-np.inf, isolated=False)
    assert list(allc.index) == list(range(-47, 48))          # [-48's window would start below -fs / 2]
    assert set(loose.index) == set(allc.index[allc.snr_db >= 10.0])
    # noise alone
    rng = np.random.default_rng(5)
    zn = 2e-3 * (rng.standard_normal(BAND_N) + 1j * rng.standard_normal(BAND_N))
    none = fc(band_row(zn), BAND_FS, BAND_FS / BAND_BINS)
    assert len(none.index) == 0 and len(none.freq_hz) == 0 and len(none.snr_db) == 0
    # an offset grid and a width
    off = fc(row, BAND_FS, 200e3, width_hz=100e3, offset_hz=100e3, min_snr_db=-np.inf, isolated=False)
    assert off.freq_hz[0] == -9.5e6 and off.index[0] == -48 and off.freq_hz[-1] == 9.5e6
    with pytest.raises(ValueError):
        fc(row, BAND_FS, 0.0)


# ---- GPU --------------------------------------------------------------------------------------
def run_dev(sdr, ctx, sp, iq, n=None, out_stride=None, rows_alloc=None, skip=0, sentinel=-7.0):
    """process_dev on a device copy of iq, the pointer advanced by `skip` complex samples; the
    whole sentinel-filled output [rows_alloc, out_stride]"""
    es = 2 if sp.u8 else 8
    n = (iq.size // 2 - skip) if n is None else n
    rows = sp.rows(n)[1]
    stride = sp.nfft if out_stride is None else out_stride
    ra = rows if rows_alloc is None else rows_alloc
    din = sdr.DeviceBuffer.from_array(ctx, iq)
    dout = sdr.DeviceBuffer.from_array(ctx, np.full(ra * stride, sentinel, np.float32))
    assert sp.process_dev(din.ptr + skip * es, n, dout.ptr, out_stride) == rows
    ctx.synchronize()
    out = dout.download(ra * stride).reshape(ra, stride)
    din.free()
    dout.free()
    return out


def against_ref(sdr, ctx, iq, nfft, hop, navg, window="hann", u8=False, what=""):
    sp = sdr.Spectrum(nfft, 1.0, hop=hop, navg=navg, window=window, iq_dtype=np.uint8 if u8 else np.float32, ctx=ctx)
    y = sp.run(iq)
    ref, bound, dg = ref_spectrum(to_complex(iq, u8), nfft, sp.hop, navg, sp.window)
    sp.close()
    return check(y, ref, bound, f"{what} nfft={nfft} hop={hop} navg={navg} {'u8' if u8 else 'f32'}", dg)


@pytest.mark.gpu
@pytest.mark.parametrize("u8", (False, True), ids=("f32", "u8"))
@pytest.mark.parametrize("nfft", SIZES)
def test_every_size(sdr, gpu_ctx, nfft, u8):
    n = 5 * nfft + 3
    for what, iq in (("noise", noise_iq(n, nfft, u8)), ("tones", tones_iq(n, nfft, u8))):
        for navg in (1, 0):
            against_ref(sdr, gpu_ctx, iq, nfft, None, navg, u8=u8, what=what)


@pytest.mark.gpu
@pytest.mark.parametrize("u8", (False, True), ids=("f32", "u8"))
@pytest.mark.parametrize("nfft", (256, 4096))
def test_hops(sdr, gpu_ctx, nfft, u8):
    for hop in (nfft // 2, nfft // 4, nfft // 2 + 1, 3, nfft + 5):
        n = nfft + 20 * hop + 1
        against_ref(sdr, gpu_ctx, noise_iq(n, hop, u8), nfft, hop, 2, u8=u8, what="hops")
        against_ref(sdr, gpu_ctx, noise_iq(n, hop, u8), nfft, hop, 0, u8=u8, what="hops")


@pytest.mark.gpu
def test_windows(sdr, gpu_ctx):
    nfft, n = 512, 512 * 7
    iq = tones_iq(n, nfft)
    rng = np.random.default_rng(8)
    for window in ("boxcar", "hann", "flattop", rng.standard_normal(nfft) + 0.2):
        against_ref(sdr, gpu_ctx, iq, nfft, nfft // 2, 3, window=window, what="window")
    assert np.min(window_of("flattop", nfft)) < 0
    # the C layer's NULL window is the Python layer's "hann"
    lib, h = gpu_ctx.lib, ctypes.c_void_p()
    sdr._lib.check(lib.sdr_spec_create(gpu_ctx.handle, nfft, None, nfft // 2, 3, 0, ctypes.byref(h)), "sdr_spec_create")
    nseg, rows = ctypes.c_int64(), ctypes.c_int64()
    assert lib.sdr_spec_rows(h, n, ctypes.byref(nseg), ctypes.byref(rows)) == 0 and (nseg.value, rows.value) == (13, 4)
    out = np.empty((4, nfft), np.float32)
    sdr._lib.check(lib.sdr_spec_run(h, iq.ctypes.data, n, out.ctypes.data, nfft), "sdr_spec_run")
    # the call-time rules, refused before any device work
    for args, word in (((nfft - 1, nfft), "< nfft"), ((nfft, nfft), "no complete row"), ((n, nfft - 1), "out_stride")):
        assert lib.sdr_spec_run(h, iq.ctypes.data, args[0], out.ctypes.data, args[1]) == -1 and word in lib.sdr_last_error().decode()
        assert lib.sdr_spec_process_dev(h, 16, args[0], 16, args[1]) == -1 and word in lib.sdr_last_error().decode()
    lib.sdr_spec_destroy(h)
    sp = sdr.Spectrum(nfft, 1.0, hop=nfft // 2, navg=3, window="hann", ctx=gpu_ctx)
    assert np.array_equal(out, sp.run(iq))
    sp.close()


@pytest.mark.gpu
def test_row_geometry(sdr, gpu_ctx):
    # 1 024 rows of one segment; one row of 4 096 segments (512 chunks of SPLIT_SEGS)
    against_ref(sdr, gpu_ctx, noise_iq(1 << 16, 20), 64, None, 1, what="1024 rows")
    against_ref(sdr, gpu_ctx, noise_iq(1 << 18, 21), 64, None, 0, what="4096 segments")
    against_ref(sdr, gpu_ctx, noise_iq(1 << 18, 22, True), 64, None, 0, u8=True, what="4096 segments")
    # chunks longer than SPLIT_SEGS: 3 x 8 x 2048 segments in one row are 2 048 chunks of 24
    against_ref(sdr, gpu_ctx, noise_iq(3 * SPLIT_SEGS * TARGET_CHUNKS * 64, 23), 64, None, 0, what="chunks of 24")
    # the split threshold: rows of SPLIT_SEGS - 1, SPLIT_SEGS (one chunk) and SPLIT_SEGS + 1 (5 + 4) segments,
    # as navg and as navg = 0
    for nfft in (128, 2048):
        for segs in (SPLIT_SEGS - 1, SPLIT_SEGS, SPLIT_SEGS + 1, 2 * SPLIT_SEGS, 2 * SPLIT_SEGS + 1):
            against_ref(sdr, gpu_ctx, noise_iq(segs * nfft, segs), nfft, None, 0, what="threshold")
            against_ref(sdr, gpu_ctx, noise_iq(3 * segs * nfft + 5, segs), nfft, None, segs, what="threshold rows")


@pytest.mark.gpu
@pytest.mark.parametrize("u8", (False, True), ids=("f32", "u8"))
def test_leftover_and_padding(sdr, gpu_ctx, u8):
    """navg = 3 with leftover segments: rows beyond the count stay untouched; out_stride =
    nfft + 7: the padding keeps its sentinel"""
    nfft, n = 256, 256 * 11 + 9
    iq = noise_iq(n, 30, u8)
    sp = sdr.Spectrum(nfft, 1.0, navg=3, iq_dtype=iq.dtype, ctx=gpu_ctx)
    assert sp.rows(n) == (11, 3)
    ref, bound, _ = ref_spectrum(to_complex(iq, u8), nfft, nfft, 3, sp.window)
    out = run_dev(sdr, gpu_ctx, sp, iq, out_stride=nfft + 7, rows_alloc=5)
    check(np.ascontiguousarray(out[:3, :nfft]), ref, bound, "leftover")
    assert np.all(out[:3, nfft:] == -7.0) and np.all(out[3:] == -7.0)
    sp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("u8", (False, True), ids=("f32", "u8"))
@pytest.mark.parametrize("hop", (64, 129))
def test_alignment(sdr, gpu_ctx, hop, u8):
    """the iq pointer advanced by one complex sample (8 B: not 16-B aligned; u8: 2 B), with an
    even and an odd hop: the reference on the shifted data"""
    nfft = 128
    n = nfft + 30 * hop
    iq = noise_iq(n + 1, 40 + hop, u8)
    sp = sdr.Spectrum(nfft, 1.0, hop=hop, navg=2, iq_dtype=iq.dtype, ctx=gpu_ctx)
    for skip in (1, 0):
        ref, bound, _ = ref_spectrum(to_complex(iq, u8)[skip:skip + n], nfft, hop, 2, sp.window)
        check(run_dev(sdr, gpu_ctx, sp, iq, n=n, skip=skip), ref, bound, f"skip {skip} hop {hop}")
    sp.close()


@pytest.mark.gpu
def test_determinism_and_run(sdr, gpu_ctx):
    """the same call twice: identical bits, for one split row and for many rows; run equals
    process_dev"""
    for n, nfft, navg in ((1 << 17, 256, 0), (1 << 16, 128, 4)):
        iq = noise_iq(n, 50)
        sp = sdr.Spectrum(nfft, 1.0, hop=nfft // 2, navg=navg, ctx=gpu_ctx)
        a, b = run_dev(sdr, gpu_ctx, sp, iq), run_dev(sdr, gpu_ctx, sp, iq)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.array_equal(a.view(np.uint32), sp.run(iq).view(np.uint32))
        sp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("u8", (False, True), ids=("f32", "u8"))
def test_run_equals_process_dev(sdr, gpu_ctx, u8):
    iq = tones_iq(4096 * 3 + 1, 4096, u8)
    sp = sdr.Spectrum(4096, 1.0, hop=1000, navg=2, iq_dtype=iq.dtype, ctx=gpu_ctx)
    assert np.array_equal(run_dev(sdr, gpu_ctx, sp, iq).view(np.uint32), sp.run(iq).view(np.uint32))
    sp.close()


@pytest.mark.gpu
def test_nan_stays_in_its_row(sdr, gpu_ctx):
    for nfft in (64, 1024, 8192):
        n = nfft * 6
        iq = noise_iq(n, 60)
        iq[2 * (2 * nfft + nfft // 3 + 1)] = np.nan          # in segment 2 = the first of row 1
        sp = sdr.Spectrum(nfft, 1.0, navg=2, ctx=gpu_ctx)
        y = sp.run(iq)
        sp.close()
        ok = iq.copy()
        ok[np.isnan(ok)] = 0.0
        ref, bound, _ = ref_spectrum(to_complex(ok), nfft, nfft, 2, window_of("hann", nfft))
        assert np.all(np.isnan(y[1]))
        check(y[[0, 2]], ref[[0, 2]], bound[[0, 2]], "beside the NaN row")


@pytest.mark.gpu
def test_64_bit_offsets(sdr, gpu_ctx):
    """a 2^28 + 4096 sample f32 buffer (just over 2 GB) that never leaves the device: zero but
    for a tone in its last 4 096 samples; hop = 2^24: 17 rows, the last shows the tone"""
    nfft, n = 4096, (1 << 28) + 4096
    sp = sdr.Spectrum(nfft, 1.0, hop=1 << 24, navg=1, ctx=gpu_ctx)
    assert sp.rows(n) == (17, 17)
    buf = sdr.DeviceBuffer(gpu_ctx, 8 * n)
    buf.zero()
    tone = interleave(0.7 * np.exp(2j * np.pi * 0.1234 * np.arange(nfft)))
    buf.upload(tone, offset=8 * (1 << 28))
    dout = sdr.DeviceBuffer.from_array(gpu_ctx, np.full(17 * nfft, -7.0, np.float32))
    assert sp.process_dev(buf.ptr, n, dout.ptr) == 17
    gpu_ctx.synchronize()
    y = dout.download(17 * nfft).reshape(17, nfft)
    buf.free()
    dout.free()
    sp.close()
    ref, bound, _ = ref_spectrum(to_complex(tone), nfft, nfft, 1, window_of("hann", nfft))
    assert np.all(y[:16] == 0.0)
    check(y[16:], ref, bound, "the last row")


@pytest.mark.gpu
@pytest.mark.parametrize("u8", (False, True), ids=("f32", "u8"))
def test_end_to_end(sdr, gpu_ctx, u8):
    """Spectrum.run -> find_channels -> FilterBank(bins=...) on the synthetic band"""
    z = band_iq(sdr)
    iq = np.clip(np.rint(128.0 + 128.0 * interleave(z).astype(np.float64)), 0, 255).astype(np.uint8) if u8 else interleave(z)
    sp = sdr.Spectrum(BAND_NFFT, BAND_FS, iq_dtype=iq.dtype, ctx=gpu_ctx)
    y = sp.run(iq)
    sp.close()
    found = sdr.find_channels(y[0], BAND_FS, BAND_FS / BAND_BINS)
    want = sdr.find_channels(band_row(to_complex(iq, u8)), BAND_FS, BAND_FS / BAND_BINS)
    assert list(found.index) == [b for b, _ in PLANTED] and list(found.index) == list(want.index)
    fb = sdr.FilterBank(BAND_BINS, BAND_FS, 8, bins=found.index, ctx=gpu_ctx)
    assert np.array_equal(found.freq_hz, fb.freqs_hz)
    fb.close()
