"""The rule of the rows' modulation meter (rtsdr.RowMeterModel, rowmeter.py) and the host helpers that
read it (modulation_report, mpx_levels), on the CPU.  tests/test_rmeter.py holds the device stage to
this rule."""
import math

import numpy as np
import pytest

import rmeter_rows as rr

FS = 240e3
K = FS / (2 * math.pi)                            # Hz of deviation per radian per sample


def demod_meter(sdr, S=1, window=12000, nbins=128):
    """the model with Receiver.modulation_meter's parameters"""
    return sdr.RowMeterModel(S, window, nbins, np.float32(FS / (2 * math.pi * 1e3)), np.float32(2 * math.pi * 75e3 / FS))


def test_reference_sine_reads_0_dbr(sdr):
    """+-19 kHz peak deviation over whole periods: 0 dBr within 1e-6 dB, no carrier offset"""
    t = np.arange(240000) / FS
    x = (19e3 / K * np.sin(2 * np.pi * 1e3 * t)).astype(np.float32)
    m = demod_meter(sdr).process(x)
    rep = sdr.modulation_report(m.records(), m.hist(), FS, 1e3)
    assert abs(rep.mpx_power_dbr[0]) < 1e-6 and abs(rep.mpx_power_dbr_call[0]) < 1e-6
    assert abs(rep.carrier_offset_hz[0]) < 1e-6
    assert abs(rep.peak_pos_hz[0] - 19e3) < 0.01 and abs(rep.peak_neg_hz[0] + 19e3) < 0.01
    assert rep.over_share[0] == 0.0 and rep.windows[0] == 20 and int(m.hist().sum()) == 20


def test_ideal_multiplex_of_synth(sdr):
    """synth.fm_mpx (audio, pilot and stereo subcarrier of fm_iq's multiplex, one second): the figures
    the rule's prototype gave"""
    x = (75e3 / K * sdr.synth.fm_mpx(240000, FS)).astype(np.float32)
    m = demod_meter(sdr).process(x)
    rep = sdr.modulation_report(m.records(), m.hist(), FS, 1e3)
    assert abs(rep.peak_pos_hz[0] - 41.05e3) <= 10.0, rep.peak_pos_hz
    assert abs(rep.peak_neg_hz[0] + 41.01e3) <= 10.0, rep.peak_neg_hz
    assert abs(rep.mpx_power_dbr[0] - 3.21) <= 0.01, rep.mpx_power_dbr
    assert abs(rep.carrier_offset_hz[0]) < 1e-3
    # every 50 ms window holds the same 2 ms period: one bin, the one of (41.05 + 41.01) / 2 kHz
    assert np.flatnonzero(m.hist()[0]).tolist() == [41] and rep.deviation_percentile(50.0)[0] == 42e3


def test_constant_row(sdr):
    c = np.float32(0.0123)
    m = demod_meter(sdr, window=100).process(np.full(1000, c, np.float32))
    r = m.records()
    rep = sdr.modulation_report(r, m.hist(), FS, 1e3)
    assert abs(rep.carrier_offset_hz[0] - float(c) * K) < 1e-9 * float(c) * K
    assert r.max[0] == c and r.min[0] == c and r.windows[0] == 10
    assert m.hist()[0, 0] == 10 and m.hist().sum() == 10
    assert np.array_equal(m.windows()[0], np.full((10, 2), c))


def test_bin_edges(sdr):
    """scale = 8: a half-span k / 8 makes float32(h scale) exactly k and lands in bin k, the float32
    below it in bin k - 1; beyond the last bin the count saturates"""
    W, NB = 64, 16
    spans = [(k, np.float32(k / 8.0)) for k in range(0, NB + 4)]
    rows = []
    for k, h in spans:
        for hh in (h, np.nextafter(h, np.float32(0))):
            w = np.zeros(W, np.float32)
            w[7], w[40] = hh, -hh
            rows.append(w)
    m = sdr.RowMeterModel(1, W, NB, 8.0, np.inf).process(np.concatenate(rows))
    want = np.zeros(NB, np.uint64)
    for k, h in spans:
        want[min(k, NB - 1)] += 1
        want[min(max(k - 1, 0), NB - 1)] += 1
    assert np.array_equal(m.hist()[0], want) and m.records().windows[0] == 2 * len(spans)


def test_nonfinite_rule_and_empty_window(sdr):
    W = 64
    x = np.linspace(-1, 1, 4 * W).astype(np.float32)
    x[3], x[70], x[200] = np.nan, np.inf, -np.inf
    x[2 * W:3 * W] = np.nan                      # window 2 has no finite sample
    x.view(np.uint32)[10] = 0x7fc12345
    fin = np.isfinite(x)
    m = sdr.RowMeterModel(1, W, 8, 1.0, 0.5).process(x)
    r = m.records()
    assert r.n[0] == fin.sum() and r.nonfinite[0] == (~fin).sum() and r.n[0] + r.nonfinite[0] == 4 * W
    assert r.over[0] == np.count_nonzero(np.abs(x[fin]) > np.float32(0.5))
    assert r.max[0] == x[fin].max() and r.min[0] == x[fin].min() and np.isfinite(r.sum[0]) and np.isfinite(r.sumsq[0])
    assert r.windows[0] == 4 and r.empty_windows[0] == 1 and m.hist().sum() == 3
    assert np.array_equal(m.windows()[0, 2], np.array([np.inf, -np.inf], np.float32))
    assert r.wcount[0] == 0 and r.wmax[0] == -np.inf and r.wmin[0] == np.inf
    # no finite sample at all
    r = sdr.RowMeterModel(1, W, 8, 1.0, 0.5).process(np.full(10, np.nan, np.float32)).records()
    assert (r.n[0], r.nonfinite[0], r.max[0], r.min[0], r.sum[0], r.wcount[0]) == (0, 10, -np.inf, np.inf, 0.0, 10)


@pytest.mark.parametrize("window", (64, 100, 12000))
def test_split_invariance(sdr, window):
    """the ragged calls of the device test against one call: histogram, counts, peaks and the carried
    window identical, the sums within the bound of rmeter_rows"""
    S = 3
    x = rr.rows_of(S, rr.STREAM, seed=1)
    one = sdr.RowMeterModel(S, window, 64, 40.0, 0.5).process(x)
    many, bound, at = sdr.RowMeterModel(S, window, 64, 40.0, 0.5), rr.SumBound(S), 0
    completed = []
    for n in rr.RAGGED:
        many.process(x[:, at:at + n])
        bound.take(x[:, at:at + n])
        completed.append(many.windows())
        at += n
    a, b = one.records(), many.records()
    assert at == rr.STREAM and b.calls[0] == len(rr.RAGGED) and a.calls[0] == 1
    for k in rr.CARRIED:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert np.array_equal(one.hist(), many.hist()) and one.hist().sum() + a.empty_windows.sum() == S * (rr.STREAM // window)
    assert np.array_equal(np.concatenate(completed, axis=1), one.windows())
    eps = 2.0 ** -52
    assert np.all(np.abs(a.total_sum - b.total_sum) <= a.total_n * eps * bound.total_abs)
    assert np.all(np.abs(a.total_sumsq - b.total_sumsq) <= a.total_n * eps * a.total_sumsq)


def test_row_meter_model_is_one_call(sdr):
    x = rr.rows_of(2, 1000, seed=2)
    r, h, w = sdr.row_meter_model(x, 100, 32, 20.0, 0.5)
    m = sdr.RowMeterModel(2, 100, 32, 20.0, 0.5).process(x)
    rr.check((r, h, w), (m.records(), m.hist(), m.windows()), rr.SumBound(2))
    assert r.calls.tolist() == [1, 1] and w.shape == (2, 10, 2)


def test_arguments(sdr):
    for args in ((0, 64), (4097, 64), (1, 63), (1, 2 ** 24 + 1), (1, 64, 0), (1, 64, 1025), (1, 64, 8, 0.0), (1, 64, 8, -1.0),
                 (1, 64, 8, np.inf), (1, 64, 8, np.nan), (1, 64, 8, 1.0, np.nan)):
        with pytest.raises(ValueError):
            sdr.RowMeterModel(*args)
        with pytest.raises(ValueError):
            sdr.RowMeter(*args)                    # checked before a context exists
    sdr.RowMeterModel(1, 64, 8, 1.0, np.inf)
    sdr.RowMeterModel(4096, 2 ** 24, 1024, 1e-30, -1.0)
    with pytest.raises(ValueError):
        sdr.RowMeterModel(2, 64).process(np.zeros((3, 10), np.float32))


def test_percentiles_of_a_hand_made_histogram(sdr):
    hist = np.array([[0, 10, 0, 30, 60, 0], [0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0]], dtype=np.uint64)
    rec = sdr.RowMeterModel(3, 64, 6).records()
    rep = sdr.modulation_report(rec, hist, FS, 1e3)
    assert rep.deviation_percentile(10.0).tolist()[0] == 2e3      # the cumulative count reaches 10 of 100 in bin 1
    assert rep.deviation_percentile(10.1)[0] == 4e3 and rep.deviation_percentile(40.0)[0] == 4e3
    assert rep.deviation_percentile(40.5)[0] == 5e3 and rep.deviation_percentile(100.0)[0] == 5e3
    assert np.isnan(rep.deviation_percentile(50.0)[1]) and rep.deviation_percentile(99.0)[2] == 1e3
    assert np.all(np.isnan(rep.carrier_offset_hz)) and np.all(np.isnan(rep.peak_pos_hz))   # no sample yet
    for p in (0.0, 100.5, -1.0):
        with pytest.raises(ValueError):
            rep.deviation_percentile(p)


def spectrogram_f64(x, w, hop):
    """the rows RowSpectrum defines (one-sided, scaling 'spectrum'), in float64, averaged over the segments"""
    nfft = len(w)
    segs = np.stack([x[s:s + nfft] for s in range(0, len(x) - nfft + 1, hop)])
    p = np.abs(np.fft.rfft(segs * w, axis=1)) ** 2 / np.sum(w) ** 2
    p[:, 1:-1] *= 2.0
    return p.mean(axis=0)


def test_mpx_levels_reads_the_pilot(sdr):
    """The float64 spectrogram of synth's ideal multiplex: pilot 0.1 x 75 kHz = 7.5 kHz.

    The tolerance, from the window.  With W(d) = sum_i w[i] exp(-2 pi i d i / nfft) the window's
    transform at d bins, a line of amplitude A that sits delta bins from its nearest bin puts
    (A / 2)^2 |W(k - delta)|^2 / sum(w)^2 into bin k, and over all bins nfft sum(w^2) / sum(w)^2 =
    the equivalent noise bandwidth times (A / 2)^2 (Parseval).  mpx_levels sums five bins and divides
    by that bandwidth, so it reads the power low by the share
        leak = 1 - sum_{|k| <= 2} |W(k - delta)|^2 / (nfft sum(w^2)),
    the amplitude by leak / 2.  The other components (the audio below 2.5 kHz, the stereo sidebands
    from 35.5 kHz on) are at least 16.5 kHz = 70 bins away and add to a summed bin at most their
    amplitude times side = max_{|d| >= 60} |W(d)| / W(0); their amplitudes total 0.81 against the
    pilot's 0.1.  |pilot_hz - 7500| <= 7500 (leak / 2 + 8.1 side): 0.02 Hz for the Hann window here."""
    nfft, hop = 1024, 512
    w = sdr.design.spectrum_window("hann", nfft)
    x = 75e3 / K * sdr.synth.fm_mpx(48000, FS)
    lev = sdr.mpx_levels(spectrogram_f64(x, w, hop), FS, nfft)
    i = np.arange(nfft)
    W = lambda d: abs(np.sum(w * np.exp(-2j * np.pi * d * i / nfft)))   # noqa: E731
    delta = 19e3 * nfft / FS - round(19e3 * nfft / FS)
    leak = 1.0 - sum(W(k - delta) ** 2 for k in range(-2, 3)) / (nfft * np.sum(w * w))
    side = max(W(d) for d in np.arange(60.0, nfft / 2, 0.25)) / W(0.0)
    tol = 7500.0 * (leak / 2 + 8.1 * side)
    assert 0.0 <= leak < 1e-4 and side < 1e-5 and tol < 0.5
    assert abs(lev.pilot_hz - 7500.0) <= tol, (lev.pilot_hz, tol)
    # the subcarrier is absent here; with it the band reads most of 0.05 x 75 kHz (a rectangular biphase symbol's main lobe)
    assert lev.rds_hz < 1.0
    xr = 75e3 / K * sdr.synth.fm_mpx(48000, FS, rds=True)
    assert 0.8 * 3750.0 < sdr.mpx_levels(spectrogram_f64(xr, w, hop), FS, nfft).rds_hz < 3750.0
    with pytest.raises(ValueError):
        sdr.mpx_levels(np.ones(100), FS, nfft)
