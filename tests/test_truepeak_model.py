"""The host rules of the true-peak meter and of loudness range (rtsdr.TruePeakModel, true_peak_report,
loudness_range, design.true_peak_fir): ITU-R BS.1770-4 annex 2 and EBU Tech 3342 / 3341.  No GPU:
tests/test_truepeak.py holds the device stage to this model bit for bit."""
import numpy as np
import pytest
from scipy import signal

FS = 48000
REF = 2.0                                         # the row amplitude of PCM full scale


def model_of(sdr, x, segment=4800, taps=None):
    """the model after one call of a single row"""
    return sdr.TruePeakModel(1, 1, segment=segment, taps=taps).process([np.asarray(x, dtype=np.float32)[None, :]])


def report_of(sdr, m):
    return sdr.true_peak_report(m.peaks(), m.sample_peaks(), m.records(), REF)


def test_the_table_is_annex_2(sdr):
    h = sdr.design.true_peak_fir()
    assert h.dtype == np.float32 and h.shape == (4, 12)
    q = h.astype(np.float64) * 8192.0
    assert np.array_equal(q, np.round(q))                                  # integers / 8192, exact in float32
    assert q[0].tolist() == [14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68]
    assert q[1].tolist() == [-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155]
    assert np.array_equal(h[2], h[1][::-1]) and np.array_equal(h[3], h[0][::-1])
    assert q.sum(axis=1).tolist() == [8205, 7971, 7971, 8205]


def test_the_model_is_upfirdn(sdr):
    """the model's segment maxima are those of scipy's polyphase interpolation with the prototype
    g[4 k + p] = h[p, k]; upfirdn sums a value's 12 terms in another order: 12 roundings of at most
    2^-53 of sum |h| max |x| each"""
    rng = np.random.default_rng(1)
    n, seg = 3 * 2048 + 77, 2048
    x = rng.standard_normal(n).astype(np.float32)
    h = sdr.design.true_peak_fir()
    y = signal.upfirdn(h.T.reshape(-1).astype(np.float64), x.astype(np.float64), up=4)[:4 * n]
    per_sample = np.max(np.abs(y.reshape(n, 4)), axis=1)
    m = model_of(sdr, x, segment=seg)
    want = np.array([per_sample[g * seg:(g + 1) * seg].max() for g in range(n // seg)])
    bound = 12 * 2.0 ** -53 * float(np.max(np.sum(np.abs(h.astype(np.float64)), axis=1))) * float(np.max(np.abs(x)))
    assert m.peaks().shape == (1, 1, 3) and np.max(np.abs(m.peaks()[0, 0] - want)) <= bound
    r = m.records()
    assert abs(r.open_peak[0, 0] - per_sample[3 * seg:].max()) <= bound and abs(r.total_peak[0, 0] - per_sample.max()) <= bound
    assert np.array_equal(m.sample_peaks()[0, 0], [np.abs(x[g * seg:(g + 1) * seg]).max() for g in range(3)])


@pytest.mark.parametrize("taps", (None, "random"))
def test_any_split_into_calls_gives_the_same_arrays(sdr, taps):
    rng = np.random.default_rng(2)
    S, n, seg = 2, 9000, 2048
    table = None if taps is None else rng.standard_normal((3, 7)).astype(np.float32)
    rows = [rng.standard_normal((S, n)).astype(np.float32) for _ in range(2)]
    rows[1][1, 4000] = np.nan
    whole = sdr.TruePeakModel(S, 2, segment=seg, taps=table).process(rows)
    for cuts in ((1, 2, 3, 4, 5, 6, 7, 11, 12, 13, 2048, 4096, 8999), sorted(rng.choice(np.arange(1, n), 9, replace=False).tolist())):
        m = sdr.TruePeakModel(S, 2, segment=seg, taps=table)
        for lo, hi in zip([0] + list(cuts), list(cuts) + [n]):
            m.process([r[:, lo:hi] for r in rows])
        assert np.array_equal(m.peaks(), whole.peaks()) and np.array_equal(m.sample_peaks(), whole.sample_peaks())
        a, b = m.records(), whole.records()
        for k in ("total_n", "total_nonfinite", "total_peak", "total_sample_peak", "segments", "open_peak", "open_sample_peak"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), k
        assert a.calls.tolist() == [[len(cuts) + 1] * 2] * S and np.array_equal(a.total_nonfinite, [[0, 0], [0, table.shape[0] * table.shape[1] if taps else 48]])


def test_an_impulse_reads_the_table(sdr):
    """an impulse a at t0 puts a h[p, k] at t0 + k: segment t0 // segment reads a max_p |h[p, k]| over the k
    that stay inside it; on a segment's last sample that is k = 0 alone, and the rest lands in the next"""
    h = sdr.design.true_peak_fir().astype(np.float64)
    seg, a = 2048, np.float32(0.37)
    col = np.max(np.abs(h), axis=0)                                        # max over the phases, per k
    for t0, inside in ((100, 12), (seg - 1, 1), (seg - 5, 5), (2 * seg - 12, 12)):
        x = np.zeros(3 * seg, dtype=np.float32)
        x[t0] = a
        m = model_of(sdr, x, segment=seg)
        g = t0 // seg
        pk = m.peaks()[0, 0]
        assert pk[g] == float(a) * col[:inside].max(), (t0, pk)
        assert pk[g + 1] == (float(a) * col[inside:].max() if inside < 12 else 0.0), (t0, pk)
        assert np.count_nonzero(pk) == (1 if inside == 12 else 2) and m.sample_peaks()[0, 0, g] == float(a)
    last = model_of(sdr, np.r_[np.zeros(seg - 1, dtype=np.float32), a], segment=seg)      # the call ends with it
    assert last.peaks()[0, 0, 0] == float(a) * col[0] and last.records().open_peak[0, 0] == 0.0
    last.process([np.zeros((1, 20), dtype=np.float32)])                                   # the history carries it over
    assert last.records().open_peak[0, 0] == float(a) * col[1:].max()


def test_a_sine_between_its_samples(sdr):
    """EBU Tech 3341's true-peak signal: a 0 dBFS sine at fs / 4 sampled 45 degrees off its crests has a
    sample peak of -3.01 dBFS; the true peak reads 0 dBTP within +0.2 / -0.4 dB"""
    t = np.arange(FS)
    m = model_of(sdr, REF * np.sin(2 * np.pi * (t / 4.0) + np.pi / 4))
    r = report_of(sdr, m)
    assert abs(r.sample_peak_dbfs[0] + 3.0103) < 1e-3
    assert -0.4 <= r.true_peak_dbtp[0] <= 0.2 and -0.4 <= r.latest_dbtp[0] <= 0.2 and -0.4 <= r.total_true_peak_dbtp[0] <= 0.2, r
    steady = 20 * np.log10(m.peaks()[0, 0, 1:].max() / REF)
    assert abs(steady - 0.045) < 5e-3 and abs(r.true_peak_dbtp[0] - 0.083) < 5e-3, (steady, r)   # what this table reads; the onset adds


def test_a_997_hz_sine_and_silence(sdr):
    t = np.arange(FS)
    r = report_of(sdr, model_of(sdr, REF * np.sin(2 * np.pi * 997.0 * t / FS)))
    assert -0.4 <= r.true_peak_dbtp[0] <= 0.2 and abs(r.true_peak_dbtp[0] - 0.009) < 5e-3 and abs(r.sample_peak_dbfs[0]) < 1e-3, r
    quiet = report_of(sdr, model_of(sdr, np.zeros(FS)))
    assert all(v[0] == -np.inf for v in quiet[:4]) and quiet.nonfinite[0] == 0
    none = report_of(sdr, model_of(sdr, np.ones(100)))                                     # no segment yet: the running maximum alone
    assert none.true_peak_dbtp[0] == -np.inf and none.latest_dbtp[0] == -np.inf and np.isfinite(none.total_true_peak_dbtp[0])


def test_a_unit_table_reads_the_sample_peak(sdr):
    x = np.random.default_rng(4).standard_normal(3 * 2048 + 5).astype(np.float32)
    m = model_of(sdr, x, segment=2048, taps=[[1.0]])
    assert np.array_equal(m.peaks(), m.sample_peaks()) and m.peaks()[0, 0, 1] == float(np.abs(x[2048:4096]).max())
    r = m.records()
    assert r.peak[0, 0] == r.sample_peak[0, 0] == float(np.abs(x).max()) and r.open_peak[0, 0] == float(np.abs(x[3 * 2048:]).max())


def test_refusals(sdr):
    for kw in (dict(nstreams=0), dict(channels=3), dict(segment=2047), dict(segment=(1 << 24) + 1), dict(taps=np.ones((9, 1))),
               dict(taps=np.ones((1, 33))), dict(taps=[[np.nan]]), dict(taps=np.ones((2, 2, 2)))):
        with pytest.raises(ValueError):
            sdr.TruePeakModel(**{"nstreams": 1, "channels": 1, **kw})
    m = sdr.TruePeakModel(2, 2)
    with pytest.raises(ValueError):
        m.process([np.zeros((2, 8))])
    with pytest.raises(ValueError):
        m.process([np.zeros((2, 8)), np.zeros((2, 9))])
    with pytest.raises(ValueError):
        sdr.true_peak_report(np.zeros((1, 1, 2)), np.zeros((1, 1, 3)), m.records())


# ---- loudness range -------------------------------------------------------------------------------
def tone_energies(sdr, levels_dbfs, seconds=20):
    """stereo 1 kHz tones, `seconds` per level, through the K-weighting: the segment energies"""
    t = np.arange(seconds * FS * len(levels_dbfs))
    amp = np.repeat([REF * 10 ** (d / 20.0) for d in levels_dbfs], seconds * FS)
    x = (amp * np.sin(2 * np.pi * 1000.0 * t / FS)).astype(np.float32)[None, :]
    return sdr.LoudnessModel(1, 2).process([x, x]).energies()


@pytest.mark.parametrize("levels, want", (((-20, -30), 10.0), ((-20, -15), 5.0), ((-40, -20), 20.0), ((-50, -35, -20, -35, -50), 15.0)))
def test_loudness_range_of_tone_sequences(sdr, levels, want):
    """EBU Tech 3342's minimum requirements, +-1 LU"""
    r = sdr.loudness_range(tone_energies(sdr, levels), 4800)
    assert abs(r.lra[0] - want) <= 1.0, r
    assert abs((r.high[0] - r.low[0]) - r.lra[0]) < 1e-12 and r.values[0] == 200 * len(levels) - 29 and 2 <= r.gated[0] <= r.values[0]


def test_loudness_range_edges(sdr):
    e = tone_energies(sdr, (-20, -30), seconds=4)                          # 80 segments: 51 short-term values
    r = sdr.loudness_range(e, 4800)
    assert r.values[0] == 51 and r.gated[0] >= 2 and r.lra[0] > 0
    one = sdr.loudness_range(e[:, :, :30], 4800)                           # one value: no range
    assert one.values[0] == 1 and one.gated[0] == 1 and one.lra[0] == 0.0 and np.isnan(one.low[0])
    none = sdr.loudness_range(e[:, :, :29], 4800)
    assert none.values[0] == 0 and none.lra[0] == 0.0
    quiet = sdr.loudness_range(e * 1e-9, 4800)                             # everything below the absolute gate
    assert quiet.values[0] == 51 and quiet.gated[0] == 0 and quiet.lra[0] == 0.0
    bad = e.copy()
    bad[0, 1, 40] = np.nan                                                 # in the runs that start at 11 .. 40
    rb = sdr.loudness_range(bad, 4800)
    assert rb.values[0] == 51 - 30 and np.isfinite(rb.lra[0]) and rb.gated[0] <= 21
    two = sdr.loudness_range(np.concatenate([e, bad]), 4800)               # per stream
    assert two.values.tolist() == [51, 21] and two.lra[0] == r.lra[0] and two.lra[1] == rb.lra[0]
    with pytest.raises(ValueError):
        sdr.loudness_range(e, 2048)
    with pytest.raises(ValueError):
        sdr.loudness_range(e[0], 4800)
