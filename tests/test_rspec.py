"""The one-sided spectrum of rows of real samples (sdr_rspec, csrc/spectrum.hip; rtsdr.RowSpectrum,
Receiver.mpx_spectrum) and the multiplex indicators on top of it (rtsdr.mpx_quality).  Parity is
against the f64 definition, N = nfft,
    X_qs[k]      = sum_{i < N} w[i] x_q[s hop + i] exp(-2 pi i k i / N),          k = 0 .. N / 2
    out[q][r][k] = c_k / (navg (sum w)^2) sum_{s in row r} |X_qs[k]|^2,   c_0 = c_{N/2} = 1, else 2
which test_reference_form pins to scipy.signal.spectrogram(..., return_onesided=True).

Tolerance: the spectrum's (tests/test_spectrum.py), carried to one-sided rows.  With
G = sum|w| max|x| over the call and d_qs[k] = 1e-6 |X_qs[k]| + 5e-7 G,
    |out - ref|[q][r][k] <= c_k mean_s(2 |X_qs[k]| d_qs[k] + d_qs[k]^2) / (sum w)^2.
test_paired_form_is_reachable_in_f32 shows without a GPU that the kernel's arithmetic -- two real
segments in one complex64 transform, folded at the end -- stays under a quarter of it.  The GPU
tests print the largest share of the bound they use."""
import ctypes

import numpy as np
import pytest
import scipy.fft
from scipy.signal import get_window, spectrogram

SPLIT_SEGS = 8        # include/sdr.h SDR_SPEC_SPLIT_SEGS: an output row of more segments may be summed in chunks
TARGET_CHUNKS = 2048  # csrc/spectrum.hip SPEC_TARGET_CHUNKS: chunks grow beyond SPLIT_SEGS once a call has more than 8 x 2048 segments
SIZES = (64, 128, 256, 512, 1024, 2048, 4096, 8192)


# ---- the f64 reference ----------------------------------------------------------------------
def geometry(n, nfft, hop, navg):
    nseg = (n - nfft) // hop + 1
    na = navg if navg > 0 else nseg
    return nseg, na, nseg // na


def weights(nfft):
    c = np.full(nfft // 2 + 1, 2.0)
    c[0] = c[-1] = 1.0
    return c


def ref_rows(x, nfft, hop, navg, w):
    """(power, its tolerance) of the rows x[nrows, n], f64: [nrows, rows, nfft / 2 + 1] each"""
    x = np.asarray(x, dtype=np.float64)
    nseg, na, rows = geometry(x.shape[1], nfft, hop, navg)
    seg = np.lib.stride_tricks.sliding_window_view(x, nfft, axis=1)[:, ::hop][:, :rows * na]
    X = np.abs(scipy.fft.rfft(seg * w, axis=-1)).reshape(x.shape[0], rows, na, nfft // 2 + 1)
    G = float(np.sum(np.abs(w)) * np.max(np.abs(x)))
    d = 1e-6 * X + 5e-7 * G
    s2 = float(np.sum(w)) ** 2
    c = weights(nfft)
    return c * np.mean(X * X, axis=2) / s2, c * np.mean(2.0 * X * d + d * d, axis=2) / s2


def check(y, ref, bound, what=""):
    share = np.abs(y.astype(np.float64) - ref) / bound
    worst = float(np.max(share))
    print(f"rspec {what}: {worst:.4f} of the bound")
    assert y.shape == ref.shape and y.dtype == np.float32
    assert worst <= 1.0, (what, worst)
    return worst


def mixed_rows(nrows, n, nfft, seed):
    """row 0: noise; row 1: full-scale tones on a bin, between two bins and near fs / 2, on a DC
    offset; row 2: noise, a tone and the fs / 2 alternation; further rows: noise"""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    x = 0.5 * rng.standard_normal((nrows, n))
    if nrows > 1:
        x[1] = 0.25 + np.cos(2 * np.pi * k * 5 / nfft) + 0.3 * np.cos(2 * np.pi * 0.123456 * k + 0.1) + 0.5 * np.cos(2 * np.pi * 0.49 * k + 0.2)
    if nrows > 2:
        x[2] = 0.1 * x[2] + 0.7 * np.cos(2 * np.pi * 0.2 * k) + 0.4 * (1.0 - 2.0 * (k & 1)) - 0.3
    return x.astype(np.float32)


def window_of(name, nfft):
    return get_window(name, nfft).astype(np.float64)


# ---- the multiplex, built directly -------------------------------------------------------------
MPX_FS = 240e3


def mpx_row(n, seed, pilot=True, stereo=True, rds=True, audio=True, sigma=2e-3):
    """synth.fm_iq's multiplex at 240 kS/s, no FM: mono + 19 kHz pilot + L-R on 38 kHz + RDS
    symbols (2 375 per second) on 57 kHz + white noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / MPX_FS
    left, right = np.sin(2 * np.pi * 1e3 * t), 0.8 * np.sin(2 * np.pi * 2.5e3 * t)
    x = sigma * rng.standard_normal(n)
    if audio:
        x += 0.45 * (left + right) / 2
    if pilot:
        x += 0.1 * np.cos(2 * np.pi * 19e3 * t)
    if stereo:
        x += 0.45 * (left - right) / 2 * np.cos(2 * np.pi * 38e3 * t)
    if rds:
        sym = rng.choice(np.array([-1.0, 1.0]), size=int(n / MPX_FS * 2375.0) + 2)
        x += 0.05 * sym[(t * 2375.0).astype(np.int64)] * np.cos(2 * np.pi * 57e3 * t)
    return x


# ---- CPU ------------------------------------------------------------------------------------
@pytest.mark.parametrize("navg", (1, 3, 0))
@pytest.mark.parametrize("hop", (256, 128, 129))
def test_reference_form(sdr, hop, navg):
    """the reference helper is scipy.signal.spectrogram(..., return_onesided=True,
    scaling='spectrum', mode='psd') averaged over groups of navg columns; freqs_hz is its axis"""
    nfft, fs, n = 256, 240e3, 256 * 11 + 77
    x = mixed_rows(3, n, nfft, 1).astype(np.float64)
    for name in ("hann", "boxcar", "flattop"):
        w = window_of(name, nfft)
        f, _, S = spectrogram(x, fs=fs, window=w, nperseg=nfft, noverlap=nfft - hop, detrend=False, return_onesided=True,
                              scaling="spectrum", mode="psd", axis=-1)
        nseg, na, rows = geometry(n, nfft, hop, navg)
        assert S.shape == (3, nfft // 2 + 1, nseg)
        want = np.moveaxis(S, 1, 2)[:, :rows * na].reshape(3, rows, na, nfft // 2 + 1).mean(axis=2)
        got = ref_rows(x, nfft, hop, navg, w)[0]
        assert got.shape == (3, rows, nfft // 2 + 1) and np.allclose(got, want, rtol=1e-10, atol=1e-18)
        sp = sdr.RowSpectrum(3, nfft, fs, hop=hop, navg=navg, window=name)
        assert np.allclose(sp.freqs_hz, f) and sp.freqs_hz[0] == 0.0 and sp.freqs_hz[-1] == fs / 2
        assert np.array_equal(sp.window, w) and sp.scale == float(np.sum(w)) ** 2
        assert sp.rows(n) == (nseg, rows)


def test_rows_and_freqs(sdr):
    R = sdr.RowSpectrum
    assert R(1, 64, 1.0).rows(64) == (1, 1)
    assert R(96, 64, 1.0, hop=10).rows(64 + 9) == (1, 1) and R(96, 64, 1.0, hop=10).rows(64 + 10) == (2, 1)
    assert R(2, 64, 1.0, hop=10, navg=1).rows(64 + 10) == (2, 2)
    assert R(2, 64, 1.0, hop=64, navg=3).rows(64 * 11 + 5) == (11, 3)          # two segments left over
    assert R(65535, 1024, 240e3, hop=512).rows(15360) == (29, 1)
    sp = R(3, 1024, 240e3)
    assert sp.hop == 1024 and sp.nrows == 3 and sp.nbins == 513
    assert sp.freqs_hz.shape == (513,) and np.array_equal(sp.freqs_hz, np.arange(513) * 234.375)
    for n, kw in ((63, {}), (64 * 2, dict(navg=3))):
        with pytest.raises(ValueError):
            R(1, 64, 1.0, **kw).rows(n)


def test_paired_form_is_reachable_in_f32(sdr):
    """the kernel's arithmetic in numpy: segments 2 p and 2 p + 1 of a row (an odd count: the last
    with zeros) as the real and imaginary part of one complex64 transform of the f32-windowed
    samples, sum |Z|^2, then (Z2[k] + Z2[N - k]) c_k / 2 -- under a quarter of the bound against
    the f64 reference"""
    worst = 0.0
    for nfft in SIZES:
        for name in ("hann", "boxcar"):
            w = sdr.design.spectrum_window(name, nfft)
            assert np.array_equal(w, window_of(name, nfft))
            for nseg in (6, 5):
                x = mixed_rows(3, nseg * nfft, nfft, nfft + nseg)
                ref, bound = ref_rows(x, nfft, nfft, 0, w)
                seg = (x.reshape(3, nseg, nfft) * w.astype(np.float32)).astype(np.float32)
                if nseg & 1:
                    seg = np.concatenate([seg, np.zeros((3, 1, nfft), np.float32)], axis=1)
                z = (seg[:, 0::2] + 1j * seg[:, 1::2]).astype(np.complex64)
                Z = scipy.fft.fft(z, axis=-1)
                assert Z.dtype == np.complex64
                Z2 = np.sum((Z.real.astype(np.float32) ** 2 + Z.imag.astype(np.float32) ** 2), axis=1, dtype=np.float32)
                fold = (Z2[:, :nfft // 2 + 1] + Z2[:, (nfft - np.arange(nfft // 2 + 1)) % nfft]) * np.float32(0.5)
                P = fold.astype(np.float64) * weights(nfft) / (nseg * np.sum(w) ** 2)
                worst = max(worst, float(np.max(np.abs(P - ref[:, 0]) / bound[:, 0])))
    print(f"paired complex64 FFT: {worst:.4f} of the bound")
    assert worst < 0.25


def test_argument_errors_before_device_work(sdr):
    """Python raises ValueError before a context exists; the C entry points refuse the same
    arguments (SDR_EINVAL with a message naming the argument) before they look at their context."""
    R = sdr.RowSpectrum
    w = np.ones(64)
    for kw in (dict(nrows=0), dict(nrows=65536), dict(nfft=32), dict(nfft=16384), dict(nfft=96), dict(hop=0),
               dict(hop=(1 << 24) + 1), dict(navg=-1), dict(window=np.r_[w[:-1], np.nan]), dict(window=np.r_[w[:32], -w[:32]]),
               dict(window=w[:63]), dict(fs=0.0)):
        with pytest.raises(ValueError):
            R(**dict(dict(nrows=2, nfft=64, fs=1.0), **kw))
    sp = R(2, 64, 1.0, navg=3)
    for n in (63, 64 * 2):                                   # n < nfft; no complete row
        with pytest.raises(ValueError):
            sp.process_dev(16, n, n, 16)
        with pytest.raises(ValueError):
            sp.run(np.zeros((2, n), np.float32))
    with pytest.raises(ValueError):
        sp.process_dev(16, 64 * 3, 64 * 3 - 1, 16)           # in_stride < n
    with pytest.raises(ValueError):
        sp.process_dev(16, 64 * 3, 64 * 3, 16, out_stride=32)
    with pytest.raises(ValueError):
        sp.run(np.zeros((3, 64 * 3), np.float32))            # three rows for an object of two
    assert sp.handle is None                                 # nothing touched a device
    lib = sdr.load_library()
    dp = ctypes.POINTER(ctypes.c_double)
    out = ctypes.c_void_p()

    def create(nrows, nfft, window, hop, navg):
        wp = None if window is None else np.asarray(window, dtype=np.float64).ctypes.data_as(dp)
        return lib.sdr_rspec_create(None, nrows, nfft, wp, hop, navg, ctypes.byref(out))
    for args, word in (((0, 64, None, 64, 1), "nrows"), ((65536, 64, None, 64, 1), "nrows"), ((2, 32, None, 32, 1), "nfft"),
                       ((2, 16384, None, 64, 1), "nfft"), ((2, 96, None, 64, 1), "nfft"), ((2, 64, None, 0, 1), "hop"),
                       ((2, 64, None, (1 << 24) + 1, 1), "hop"), ((2, 64, None, 64, -1), "navg"),
                       ((2, 64, np.r_[w[:-1], np.inf], 64, 1), "window[63]"), ((2, 64, np.r_[w[:32], -w[:32]], 64, 1), "window sums"),
                       ((2, 64, None, 64, 1), "context is NULL"), ((65535, 8192, w.repeat(128), 1, 0), "context is NULL")):
        assert create(*args) == -1 and word in lib.sdr_last_error().decode(), (args, lib.sdr_last_error())
    assert lib.sdr_rspec_create(None, 2, 64, None, 64, 1, None) == -1 and "out" in lib.sdr_last_error().decode()
    assert lib.sdr_rspec_process_dev(None, None, 64, 64, None, 64) == -1 and "NULL" in lib.sdr_last_error().decode()
    assert lib.sdr_rspec_run(None, None, 64, 64, None, 64) == -1 and "NULL" in lib.sdr_last_error().decode()
    assert lib.sdr_rspec_rows(None, 64, None, None) == -1 and "NULL" in lib.sdr_last_error().decode()


def mpx_spectra(rows, nfft):
    x = np.stack(rows)
    return ref_rows(x, nfft, nfft // 2, 0, window_of("hann", nfft))[0][:, 0]


@pytest.mark.parametrize("nfft", (512, 1024, 4096))
def test_mpx_quality(sdr, nfft):
    n = 15360
    p = mpx_spectra([mpx_row(n, 1), mpx_row(n, 2, pilot=False, stereo=False, rds=False),
                     mpx_row(n, 3, pilot=False, stereo=False, rds=False, audio=False)], nfft)
    q = sdr.mpx_quality(p)
    print(f"mpx_quality nfft={nfft}: pilot {np.round(q.pilot_snr_db, 1)} dB, rds {np.round(q.rds_snr_db, 1)} dB")
    assert isinstance(q, sdr.MpxQuality) and q._fields == ("pilot_snr_db", "rds_snr_db", "noise_floor", "stereo", "rds")
    assert list(q.stereo) == [True, False, False] and list(q.rds) == [True, False, False]
    assert q.pilot_snr_db.shape == (3,) and q.stereo.dtype == bool and q.rds.dtype == bool
    # the definition, spelled out for row 0
    f = np.arange(nfft // 2 + 1) * (MPX_FS / nfft)
    band = (f >= 18.5e3) & (f <= 19.5e3)
    guard = ((f >= 16e3) & (f <= 18e3)) | ((f >= 20e3) & (f <= 22e3))
    floor = np.median(p[0][guard])
    assert np.isclose(q.noise_floor[0], floor, rtol=1e-12)
    assert np.isclose(q.pilot_snr_db[0], 10 * np.log10(np.sum(p[0][band]) / (floor * np.count_nonzero(band))), rtol=1e-12)
    rband, rguard = (f >= 55e3) & (f <= 59e3), (f >= 60e3) & (f <= 64e3)
    assert np.isclose(q.rds_snr_db[0], 10 * np.log10(np.sum(p[0][rband]) / (np.median(p[0][rguard]) * np.count_nonzero(rband))),
                      rtol=1e-12)
    # white noise of variance sigma^2 through a Hann window: sigma^2 sum w^2 / (sum w)^2 per two-sided bin, twice that one-sided
    w = window_of("hann", nfft)
    assert 0.5 < q.noise_floor[2] / (2 * 2e-3 ** 2 * np.sum(w * w) / np.sum(w) ** 2) < 2.0
    assert np.all(np.abs(q.pilot_snr_db[1:]) < 6.0) and np.all(np.abs(q.rds_snr_db[1:]) < 4.0)
    # thresholds, shapes
    one = sdr.mpx_quality(p[0])
    assert one.pilot_snr_db.shape == () and bool(one.stereo) and bool(one.rds)
    assert one.pilot_snr_db == q.pilot_snr_db[0]
    strict = sdr.mpx_quality(p, min_pilot_db=80.0, min_rds_db=80.0)
    assert not strict.stereo.any() and not strict.rds.any()
    assert sdr.mpx_quality(p.reshape(3, 1, -1)).stereo.shape == (3, 1)


def test_mpx_quality_refuses_wide_bins(sdr):
    with pytest.raises(ValueError):
        sdr.mpx_quality(np.ones(129))                        # nfft 256 at 240 kHz: 937.5 Hz
    with pytest.raises(ValueError):
        sdr.mpx_quality(np.ones(513), fs=128e3)              # fs / 2 = 64 kHz: the RDS guard does not fit
    with pytest.raises(ValueError):
        sdr.mpx_quality(np.ones(513), fs=1e6)                # 976 Hz
    assert sdr.mpx_quality(np.ones(257)).pilot_snr_db == 0.0     # nfft 512: 468.75 Hz


# ---- GPU --------------------------------------------------------------------------------------
def run_dev(sdr, ctx, sp, x, gap=5, lead=1, out_pad=0, rows_alloc=None, sentinel=-7.0):
    """process_dev on a device copy of the rows x[nrows, n] laid out in_stride = n + gap floats
    apart, `lead` floats into the buffer; the lead, the gaps and a tail are NaN.  Returns the whole
    sentinel-filled output [rows_alloc, nbins + out_pad]."""
    nrows, n = x.shape
    rows = sp.rows(n)[1]
    stride = n + gap
    buf = np.full(lead + nrows * stride + 64, np.nan, np.float32)
    for q in range(nrows):
        buf[lead + q * stride:lead + q * stride + n] = x[q]
    ostride = sp.nbins + out_pad
    ra = nrows * rows if rows_alloc is None else rows_alloc
    din = sdr.DeviceBuffer.from_array(ctx, buf)
    dout = sdr.DeviceBuffer.from_array(ctx, np.full(ra * ostride, sentinel, np.float32))
    assert sp.process_dev(din.ptr + 4 * lead, n, stride, dout.ptr, ostride if out_pad else None) == rows
    ctx.synchronize()
    out = dout.download(ra * ostride).reshape(ra, ostride)
    din.free()
    dout.free()
    return out


def against_ref(sdr, ctx, x, nfft, hop, navg, window="hann", what="", out_pad=3):
    """process_dev on strided, NaN-surrounded rows against the f64 reference; the padding of the
    output rows keeps its sentinel"""
    sp = sdr.RowSpectrum(x.shape[0], nfft, 1.0, hop=hop, navg=navg, window=window, ctx=ctx)
    out = run_dev(sdr, ctx, sp, x, out_pad=out_pad)
    ref, bound = ref_rows(x, nfft, sp.hop, navg, sp.window)
    y = np.ascontiguousarray(out[:, :sp.nbins]).reshape(ref.shape)
    sp.close()
    assert np.all(np.isfinite(y)), what                      # no NaN from a gap or from the tail was read
    assert np.all(out[:, sp.nbins:] == -7.0), what
    return check(y, ref, bound, f"{what} nfft={nfft} hop={hop} navg={navg} rows={x.shape[0]}")


@pytest.mark.gpu
@pytest.mark.parametrize("nfft", SIZES)
def test_every_size(sdr, gpu_ctx, nfft):
    """3 rows in_stride = n + 5 apart from an odd float offset on: rows at odd 4-byte alignments"""
    segs = 5 + SIZES.index(nfft) % 5                          # 5 .. 9
    n = segs * nfft + 3
    x = mixed_rows(3, n, nfft, nfft)
    for hop, navg in ((None, 0), (None, 1), (nfft // 2, 2)):
        against_ref(sdr, gpu_ctx, x, nfft, hop, navg, what="size")


@pytest.mark.gpu
def test_odd_navg_and_odd_chunks(sdr, gpu_ctx):
    """navg = 3 and 5: the last segment of every output row is paired with zeros.  A row of 19
    segments is cut at SPLIT_SEGS = 8 into chunks of 7, 7 and 5: pairs end on zeros inside chunks.
    Rows of SPLIT_SEGS - 1 .. 2 SPLIT_SEGS + 1 segments: either side of the split."""
    for nfft in (128, 2048):
        x = mixed_rows(3, 19 * nfft + 7, nfft, 70)
        for navg in (3, 5, 19, 0):
            against_ref(sdr, gpu_ctx, x, nfft, None, navg, what="odd")
        against_ref(sdr, gpu_ctx, mixed_rows(2, nfft + 18 * (nfft // 2), nfft, 71), nfft, nfft // 2, 0, what="19 overlapped")
        for segs in (SPLIT_SEGS - 1, SPLIT_SEGS, SPLIT_SEGS + 1, 2 * SPLIT_SEGS, 2 * SPLIT_SEGS + 1):
            against_ref(sdr, gpu_ctx, mixed_rows(2, 2 * segs * nfft + 5, nfft, segs), nfft, None, segs, what="threshold")


@pytest.mark.gpu
@pytest.mark.parametrize("nfft", (256, 4096))
def test_hops(sdr, gpu_ctx, nfft):
    for hop in (nfft // 2 + 1, 3, 1, nfft + 5, 3 * nfft + 1):
        x = mixed_rows(3, nfft + 20 * hop + 1, nfft, hop)
        against_ref(sdr, gpu_ctx, x, nfft, hop, 2, what="hops")
        against_ref(sdr, gpu_ctx, x, nfft, hop, 0, what="hops")


@pytest.mark.gpu
def test_windows_and_call_rules(sdr, gpu_ctx):
    nfft, n = 512, 512 * 7
    x = mixed_rows(2, n, nfft, 8)
    rng = np.random.default_rng(8)
    for window in ("boxcar", "hann", "flattop", rng.standard_normal(nfft) + 0.2):
        against_ref(sdr, gpu_ctx, x, nfft, nfft // 2, 3, window=window, what="window")
    # the C layer's NULL window is the Python layer's "hann"
    lib, h = gpu_ctx.lib, ctypes.c_void_p()
    sdr._lib.check(lib.sdr_rspec_create(gpu_ctx.handle, 2, nfft, None, nfft // 2, 3, ctypes.byref(h)), "sdr_rspec_create")
    nseg, rows = ctypes.c_int64(), ctypes.c_int64()
    assert lib.sdr_rspec_rows(h, n, ctypes.byref(nseg), ctypes.byref(rows)) == 0 and (nseg.value, rows.value) == (13, 4)
    nb = nfft // 2 + 1
    out = np.empty((2, 4, nb), np.float32)
    sdr._lib.check(lib.sdr_rspec_run(h, x.ctypes.data, n, n, out.ctypes.data, nb), "sdr_rspec_run")
    # the call-time rules, refused before any device work
    for (cn, cis, cos), word in (((nfft - 1, n, nb), "< nfft"), ((nfft, n, nb), "no complete row"), ((n, n - 1, nb), "in_stride"),
                                 ((n, n, nb - 1), "out_stride")):
        assert lib.sdr_rspec_run(h, x.ctypes.data, cn, cis, out.ctypes.data, cos) == -1 and word in lib.sdr_last_error().decode()
        assert lib.sdr_rspec_process_dev(h, 16, cn, cis, 16, cos) == -1 and word in lib.sdr_last_error().decode()
    for xp, op in ((18, 16), (16, 17)):
        assert lib.sdr_rspec_process_dev(h, xp, n, n, op, nb) == -1 and "aligned" in lib.sdr_last_error().decode()
    lib.sdr_rspec_destroy(h)
    sp = sdr.RowSpectrum(2, nfft, 1.0, hop=nfft // 2, navg=3, window="hann", ctx=gpu_ctx)
    assert np.array_equal(out, sp.run(x))
    sp.close()


@pytest.mark.gpu
def test_long_call(sdr, gpu_ctx):
    """3 rows of 6 000 segments at nfft 64, hop 1: 18 000 > 8 x 2 048 segments in the call, so the
    chunks grow to ceil(18 000 / 2 048) = 9 segments -- counted over all rows; a row alone would
    stay at 8 -- and every row is 667 chunks of odd length.  And many output rows: 500 per row."""
    nfft, n = 64, 64 + 5999
    x = mixed_rows(3, n, nfft, 90)
    assert 3 * 6000 > SPLIT_SEGS * TARGET_CHUNKS > 6000
    against_ref(sdr, gpu_ctx, x, nfft, 1, 0, what="long")
    against_ref(sdr, gpu_ctx, x, nfft, 1, 12, what="500 rows per row")


@pytest.mark.gpu
def test_determinism_and_run(sdr, gpu_ctx):
    """the same call twice: identical bits, for split rows and for many rows; run (packed rows)
    equals process_dev (strided rows at another alignment)"""
    for n, nfft, navg in ((1 << 14, 256, 0), (1 << 13, 128, 5), (3 * 4096 + 1, 4096, 0)):
        x = mixed_rows(3, n, nfft, 50)
        sp = sdr.RowSpectrum(3, nfft, 1.0, hop=nfft // 2, navg=navg, ctx=gpu_ctx)
        a, b = run_dev(sdr, gpu_ctx, sp, x), run_dev(sdr, gpu_ctx, sp, x)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        y = sp.run(x)
        assert y.shape == (3, sp.rows(n)[1], sp.nbins)
        assert np.array_equal(a.view(np.uint32).reshape(-1), y.view(np.uint32).reshape(-1))
        sp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nfft", (64, 256, 8192))
def test_nan_stays_in_its_rows(sdr, gpu_ctx, nfft):
    """hop = nfft / 2, navg = 3, 10 segments per row: 3 output rows and a leftover segment.  One
    NaN sample changes exactly the output rows whose segments contain it: all of their bins are
    NaN, every other row keeps its bits."""
    hop, nrows = nfft // 2, 3
    n = nfft + 9 * hop + 5
    x = mixed_rows(nrows, n, nfft, 60)
    sp = sdr.RowSpectrum(nrows, nfft, 1.0, hop=hop, navg=3, ctx=gpu_ctx)
    assert sp.rows(n) == (10, 3)
    clean = sp.run(x)
    assert np.all(np.isfinite(clean))
    # (row, sample) -> the output rows hit: segments 2 and 3 -> rows 0 and 1; segment 0 -> row 0;
    # segments 8 and 9 -> row 2; segment 9 alone (the leftover, and the tail no segment covers) -> none
    for (q, p), hit in (((1, 3 * hop + 10), (0, 1)), ((0, 3), (0,)), ((2, 9 * hop + 1), (2,)), ((1, 9 * hop + hop + 1), ()),
                        ((0, n - 1), ())):
        segs = [s for s in range(10) if s * hop <= p < s * hop + nfft]
        assert tuple(sorted({s // 3 for s in segs if s < 9})) == hit
        bad = x.copy()
        bad[q, p] = np.nan
        y = sp.run(bad)
        for qq in range(nrows):
            for r in range(3):
                if qq == q and r in hit:
                    assert np.all(np.isnan(y[qq, r])), (q, p, qq, r)
                else:
                    assert np.array_equal(y[qq, r].view(np.uint32), clean[qq, r].view(np.uint32)), (q, p, qq, r)
    sp.close()


@pytest.mark.gpu
def test_receiver_end_to_end(sdr, gpu_ctx):
    """two streams through a Receiver -- an FM station at 30 dB SNR and noise alone --, the second
    block's "demod" rows through Receiver.mpx_spectrum(1024).process_rx, read in place: the f64
    reference of the fetched rows within the bound, and mpx_quality lights the lamps of stream 0
    only"""
    B = 51200
    iq = np.stack([sdr.synth.fm_iq(2 * B, seed=0, snr_db=30.0), sdr.synth.fm_iq(2 * B, seed=1, snr_db=-40.0)])
    rx = sdr.Receiver(2, B, mono=True, iq_dtype=np.float32, ctx=gpu_ctx)
    sp = rx.mpx_spectrum(1024)
    assert (sp.nrows, sp.nfft, sp.hop, sp.navg, sp.fs) == (2, 1024, 512, 0, 240e3)
    for k in range(2):
        rx.process(iq[:, 2 * B * k:2 * B * (k + 1)])
    _, _, n = rx.output_ptr("demod")
    assert n == B // 10 and sp.rows(n) == (9, 1)
    dout = sdr.DeviceBuffer.from_array(gpu_ctx, np.full(2 * sp.nbins, -7.0, np.float32))
    assert sp.process_rx(rx, dout.ptr) == 1
    gpu_ctx.synchronize()
    y = dout.download(2 * sp.nbins).reshape(2, 1, sp.nbins)
    dout.free()
    demod = rx.output("demod")
    ref, bound = ref_rows(demod, 1024, 512, 0, sp.window)
    check(y, ref, bound, "receiver demod rows")
    q = sdr.mpx_quality(y[:, 0], fs=sp.fs)
    print(f"rspec end to end: pilot {np.round(q.pilot_snr_db, 1)} dB, rds {np.round(q.rds_snr_db, 1)} dB")
    assert list(q.stereo) == [True, False] and list(q.rds) == [True, False]
    with pytest.raises(ValueError):                          # a spectrum of three rows on a receiver of two streams
        sdr.RowSpectrum(3, 1024, 240e3, ctx=gpu_ctx).process_rx(rx, 16)
    sp.close()
    rx.close()
