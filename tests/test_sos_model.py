"""The host rules of the cascade of second-order sections and of the loudness meter
(rtsdr.sos_model, LoudnessModel, loudness_report, design.k_weighting_sos, pilot_notch_sos), and the C
entry points' refusals (csrc/sos.hip), which come before the context check: no GPU is needed."""
import ctypes

import numpy as np
import pytest
from scipy import signal

import sos_rows as sr

FS = 48000.0
REF = 2.0            # the row amplitude of PCM full scale (int16(x * 16384))


class LoudParams(ctypes.Structure):
    _fields_ = [("segment", ctypes.c_int64), ("cap", ctypes.c_int), ("reference", ctypes.c_double)]


def sine(seconds, amplitude, f=997.0):
    return (amplitude * np.sin(2 * np.pi * f * np.arange(int(seconds * FS)) / FS)).astype(np.float32)


def k_gain_db(sdr, f=997.0):
    _, h = signal.sosfreqz(sdr.design.k_weighting_sos(), worN=[f], fs=FS)
    return 20 * np.log10(abs(h[0]))


# ---- sos_model ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sr.SETS)
def test_sos_model_is_sosfilt_rounded_once_and_carries_its_state(sdr, name):
    sos = sr.coefficient_sets()[name]
    x = sr.rows_of(5000)
    y, zf = sdr.sos_model(sos, x)
    want, wz = signal.sosfilt(sos, x.astype(np.float64), axis=-1, zi=np.zeros((sos.shape[0], sr.S, 2)))
    assert y.dtype == np.float32 and np.array_equal(y, want.astype(np.float32))
    assert zf.dtype == np.float64 and zf.shape == (sr.S, sos.shape[0], 2) and np.array_equal(zf, wz.transpose(1, 0, 2))
    parts, z = [], None
    for lo, hi in ((0, 1), (1, 2048), (2048, 4097), (4097, 5000)):
        p, z = sdr.sos_model(sos, x[:, lo:hi], zi=z)
        parts.append(p)
    assert np.array_equal(np.concatenate(parts, axis=1), y) and np.array_equal(z, zf)
    y1, z1 = sdr.sos_model(sos, x[1])                                  # one row, one dimension
    assert np.array_equal(y1[0], y[1]) and np.array_equal(z1[0], zf[1])


def test_sos_model_refuses_what_the_device_refuses(sdr):
    x = np.ones((1, 8), np.float32)
    for sos in ([[1, 0, 0, 2, 0, 0]], [[1, 0, 0, 1, 0, 1.0]], [[1, 0, 0, 1, 2.0, 0.99]], [[1, 0, 0, 1, -1.5, 0.5]], [[np.nan, 0, 0, 1, 0, 0]],
                np.tile([1.0, 0, 0, 1, 0, 0], (5, 1)), [[1, 0, 0, 1, 0]]):
        with pytest.raises(ValueError):
            sdr.sos_model(sos, x)
    sdr.sos_model([[1, 0, 0, 1, -1.98, 0.9801]], x)                    # a double pole at 0.99: inside


# ---- the designs ----------------------------------------------------------------------------------
def test_k_weighting_is_the_standards_table(sdr):
    sos = sdr.design.k_weighting_sos()
    assert sos.shape == (2, 6) and np.array_equal(sos, sr.coefficient_sets()["k_weighting"])
    assert abs(k_gain_db(sdr) - 0.691) < 1e-3                          # what the -0.691 of the loudness formula undoes
    for fs in (44100.0, 96e3, 0.0):
        with pytest.raises(ValueError):
            sdr.design.k_weighting_sos(fs)


def test_pilot_notch(sdr):
    sos = sdr.design.pilot_notch_sos()
    assert sos.shape == (1, 6) and np.array_equal(sos, signal.tf2sos(*signal.iirnotch(19e3, 30, 48e3)))
    _, h = signal.sosfreqz(sos, worN=[1e3, 15e3, 19e3], fs=FS)
    assert abs(h[2]) < 1e-10 and abs(abs(h[0]) - 1) < 1e-3 and abs(h[1]) > 0.97


# ---- loudness -------------------------------------------------------------------------------------
def test_full_scale_997_hz_sine_reads_minus_3_01_lufs(sdr):
    """BS.1770's calibration: a 0 dBFS 997 Hz sine in one channel, the other silent; both: 3.01 LU more"""
    x = sine(5.0, REF)[None, :]
    want = -0.691 + k_gain_db(sdr) + 10 * np.log10(0.5)                # the sine's mean square is 1/2 of full scale's square
    assert abs(want + 3.0107) < 1e-3
    one = sdr.LoudnessModel(1, 2).process([x, np.zeros_like(x)])
    e = one.energies()
    assert e.shape == (1, 2, 50) and one.pos == 240000
    settled = -0.691 + 10 * np.log10((e[0, 0, 10:-3] + e[0, 0, 11:-2] + e[0, 0, 12:-1] + e[0, 0, 13:]) / 19200.0)
    assert np.all(np.abs(settled - want) < 2e-3)                       # 398.8 cycles a block: the mean square ripples by 4e-4
    # the exact value of each settled block: the steady-state response from sosfreqz, summed over the block's own samples
    _, h = signal.sosfreqz(sdr.design.k_weighting_sos(), worN=[997.0], fs=FS)
    steady = abs(h[0]) * np.sin(2 * np.pi * 997.0 * np.arange(240000) / FS + np.angle(h[0]))
    seg = np.sum(steady.reshape(50, 4800) ** 2, axis=1)
    exact = -0.691 + 10 * np.log10((seg[10:-3] + seg[11:-2] + seg[12:-1] + seg[13:]) / 19200.0)
    assert np.all(np.abs(settled - exact) < 1e-6 * np.abs(exact)), np.max(np.abs(settled - exact))
    r = sdr.loudness_report(e, 4800)
    assert abs(r.momentary[0] + 3.01) < 0.02 and abs(r.short_term[0] + 3.01) < 0.02 and abs(r.integrated[0] + 3.01) < 0.02
    assert r.blocks[0] == 47 and r.nonfinite_blocks[0] == 0
    both = sdr.loudness_report(sdr.LoudnessModel(1, 2).process([x, x]).energies(), 4800)
    assert abs(both.integrated[0] - r.integrated[0] - 3.0103) < 1e-3 and abs(both.momentary[0] - r.momentary[0] - 3.0103) < 1e-3
    mono = sdr.loudness_report(sdr.LoudnessModel(1, 1).process([x]).energies(), 4800)
    assert abs(mono.integrated[0] - r.integrated[0]) < 1e-9


def test_gating_and_silence(sdr):
    """20 s at -23 LUFS then 20 s at -60: the relative gate leaves the quiet part out; silence reads -inf"""
    g = k_gain_db(sdr)
    amp = lambda lufs: REF * np.sqrt(2.0) * 10 ** ((lufs + 0.691 - g) / 20)   # noqa: E731  a mono sine of that loudness
    x = np.concatenate([sine(20.0, amp(-23.0)), sine(20.0, amp(-60.0))])
    rows = np.stack([x, np.zeros_like(x)])                             # stream 1: digital silence
    m = sdr.LoudnessModel(2, 1)
    for lo in range(0, x.size, 100_003):                               # carried across ragged calls
        m.process([rows[:, lo:lo + 100_003]])
    r = sdr.loudness_report(m.energies(), 4800)
    assert abs(r.integrated[0] + 23.0) < 0.1, r.integrated
    assert abs(r.momentary[0] + 60.0) < 0.1 and abs(r.short_term[0] + 60.0) < 0.1
    assert r.blocks[0] == 397 and 190 <= r.gated_blocks[0] <= 200
    assert r.integrated[1] == -np.inf and r.momentary[1] == -np.inf and r.short_term[1] == -np.inf and r.gated_blocks[1] == 0
    e = m.energies().copy()
    e[0, 0, 5] = np.nan                                                # four blocks hold segment 5
    rn = sdr.loudness_report(e, 4800)
    assert rn.nonfinite_blocks[0] == 4 and abs(rn.integrated[0] + 23.0) < 0.1
    few = sdr.loudness_report(e[:, :, :3], 4800)                       # no block yet
    assert few.blocks[0] == 0 and few.integrated[0] == -np.inf and few.momentary[0] == -np.inf
    with pytest.raises(ValueError):
        sdr.loudness_report(e, 2048)                                   # not 100 ms


def test_model_and_meter_arguments(sdr):
    for kw in (dict(nstreams=0), dict(nstreams=4097), dict(channels=0), dict(channels=3), dict(segment=2047), dict(segment=2 ** 24 + 1),
               dict(reference=0.0), dict(reference=np.inf), dict(reference=-2.0)):
        a = dict(nstreams=1, channels=1)
        a.update(kw)
        with pytest.raises(ValueError):
            sdr.LoudnessModel(**a)
        with pytest.raises(ValueError):
            sdr.LoudnessMeter(**a)                                     # no context is made for a refusal
    for kw in (dict(cap=3), dict(cap=2 ** 20 + 1)):
        with pytest.raises(ValueError):
            sdr.LoudnessMeter(1, **kw)
    with pytest.raises(ValueError):
        sdr.RowSos(0, sdr.design.k_weighting_sos())
    with pytest.raises(ValueError):
        sdr.RowSos(1, [[1, 0, 0, 1, 0, 1.0]])
    assert sdr.RowSos(4096, sdr.design.k_weighting_sos()).K == 2 and sdr.RowSos.TILE == sr.TILE


# ---- the C entry points' refusals: no GPU, the library loaded, ctx = NULL --------------------------
def test_c_entry_points_refuse_bad_arguments_before_the_context(sdr):
    lib = sdr.load_library()
    out = ctypes.c_void_p()
    err = lambda: lib.sdr_last_error().decode()                        # noqa: E731
    good = [1.0, 0.0, 0.0, 1.0, -0.5, 0.25]

    def create(nrows=1, sos=good, K=1, out_ref=ctypes.byref(out)):
        a = None if sos is None else (ctypes.c_double * len(sos))(*sos)
        return lib.sdr_sos_create(None, nrows, a, K, out_ref)
    for kw, word in ((dict(out_ref=None), "out is NULL"), (dict(sos=None), "sos is NULL"), (dict(nrows=0), "nrows"), (dict(nrows=4097), "nrows"),
                     (dict(K=0), "K="), (dict(K=5, sos=good * 5), "K="), (dict(sos=[np.nan] + good[1:]), "not finite"),
                     (dict(sos=good[:5] + [np.inf]), "not finite"), (dict(sos=[1.0, 0, 0, 2.0, 0, 0]), "a0"), (dict(sos=[1.0, 0, 0, 1, 0, 1.0]), "pole"),
                     (dict(sos=[1.0, 0, 0, 1, 0, -1.0]), "pole"), (dict(sos=[1.0, 0, 0, 1, 1.5, 0.5]), "pole"), (dict(sos=[1.0, 0, 0, 1, -1.6, 0.5]), "pole"),
                     (dict(sos=good + [1.0, 0, 0, 1, 2.0, 1.0], K=2), "section 1"), (dict(), "context is NULL"),
                     (dict(nrows=4096, K=4, sos=good * 4), "context is NULL")):
        assert create(**kw) == -1 and word in err(), (kw, err())
    assert lib.sdr_sos_process_dev(None, None, 8, None, 8, 8) == -1 and "NULL" in err()
    assert lib.sdr_sos_run(None, None, None, 8, 8) == -1 and "NULL" in err()
    assert lib.sdr_sos_reset(None) == -1 and lib.sdr_sos_state(None, None) == -1 and lib.sdr_sos_set_state(None, None) == -1
    assert lib.sdr_sos_set_timing(None, 1) == -1 and lib.sdr_sos_stage_ms(None, None) == -1
    lib.sdr_sos_destroy(None)

    def loud(S=1, channels=2, segment=4800, cap=64, reference=2.0, prm=True, out_ref=ctypes.byref(out)):
        return lib.sdr_loud_create(None, S, channels, ctypes.byref(LoudParams(segment, cap, reference)) if prm else None, out_ref)
    for kw, word in ((dict(out_ref=None), "out is NULL"), (dict(prm=False), "params is NULL"), (dict(S=0), "nstreams"), (dict(S=4097), "nstreams"),
                     (dict(channels=0), "channels"), (dict(channels=3), "channels"), (dict(segment=2047), "segment"), (dict(segment=2 ** 24 + 1), "segment"),
                     (dict(cap=3), "cap"), (dict(reference=0.0), "reference"), (dict(reference=-1.0), "reference"), (dict(reference=np.nan), "reference"),
                     (dict(reference=np.inf), "reference"), (dict(), "context is NULL"), (dict(S=4096, channels=1, segment=2048, cap=4), "context is NULL")):
        assert loud(**kw) == -1 and word in err(), (kw, err())
    assert lib.sdr_loud_process_dev(None, None, None, 8, 8) == -1 and "NULL" in err()
    assert lib.sdr_loud_run(None, None, None, 8, 8) == -1 and "NULL" in err()
    assert lib.sdr_loud_reset(None) == -1 and lib.sdr_loud_segments(None, None, None, None) == -1 and lib.sdr_loud_state_dev(None, None, None) == -1
    assert lib.sdr_loud_set_timing(None, 1) == -1 and lib.sdr_loud_stage_ms(None, None) == -1
    lib.sdr_loud_destroy(None)
