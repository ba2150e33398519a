"""fm_radio_gpu --deemph 50|75: FM de-emphasis and the int16 conversion on the device (the
receiver's audio output stage in mode 0, sdr_audio_out_dev in mode 1); only the PCM comes back.
The reference has no de-emphasis: the PCM is compared with the reference writer's rule
(tests/test_live.py to_pcm) applied to scipy's de-emphasis, in f64, of the concatenated block
outputs of the Python API, with the existing live tests' acceptance (<= 1 LSB, < 1 % off)."""
import subprocess

import numpy as np
import pytest
from scipy import signal

from test_live import B, BIN, to_pcm


def deemph(sdr, x, tau):
    b, a = sdr.design.deemphasis_coeffs(tau, 48e3)
    return signal.lfilter(b, a, np.asarray(x, dtype=np.float32).astype(np.float64))


def accept(pcm, ref):
    assert pcm.shape == ref.shape
    d = np.abs(pcm.astype(np.int32) - ref)
    print(f"int16: max |diff| {d.max()}, {np.mean(d > 0) * 100:.4f} % off by one")
    assert d.max() <= 1 and np.mean(d > 0) < 0.01


def test_deemph_usage_errors():
    assert subprocess.run([BIN, "--deemph", "60"], capture_output=True).returncode == 2
    assert subprocess.run([BIN, "--deemph"], capture_output=True).returncode == 2
    assert subprocess.run([BIN, "--deemph", "75us"], capture_output=True).returncode == 2


def test_print_taps_is_unchanged_by_the_flag():
    plain = subprocess.run([BIN, "--print-taps"], capture_output=True, text=True, check=True).stdout
    res = subprocess.run([BIN, "--print-taps", "--deemph", "75"], capture_output=True, text=True, check=True)
    assert res.stdout == plain and len(plain.splitlines()) == 11


@pytest.mark.gpu
def test_live_deemph_stereo(sdr, gpu_ctx):
    nb = 4
    iq = sdr.synth.fm_iq(nb * B, seed=9, dtype=np.uint8)
    res = subprocess.run([BIN, "--deemph", "75"], input=iq.tobytes() + b"\x80" * 1000, capture_output=True, check=True,
                         timeout=120)
    pcm = np.frombuffer(res.stdout, dtype=np.int16)
    assert pcm.shape == (nb * 2 * (B // 50),)              # the output length is unchanged
    rf, au = sdr.design.mono_coeffs(151, 151)
    proc = sdr.StereoBlockProcessor(B, rf, au, iq_dtype=np.uint8)
    outs = [proc.process(iq[2 * k * B:2 * (k + 1) * B]) for k in range(nb)]
    left = np.concatenate([o["left"] for o in outs])
    right = np.concatenate([o["right"] for o in outs])
    accept(pcm, to_pcm(deemph(sdr, left, 75e-6), deemph(sdr, right, 75e-6)))
    # the de-emphasis is there: the plain run differs, and by more at the top of the band
    plain = np.frombuffer(subprocess.run([BIN], input=iq.tobytes(), capture_output=True, check=True,
                                         timeout=120).stdout, dtype=np.int16)
    assert plain.shape == pcm.shape and not np.array_equal(plain, pcm)


@pytest.mark.gpu
def test_live_deemph_mono_50us(sdr, gpu_ctx):
    nb = 4
    iq = sdr.synth.fm_iq(nb * B, seed=12, dtype=np.uint8)
    res = subprocess.run([BIN, "--deemph", "50", "--mono"], input=iq.tobytes(), capture_output=True, check=True,
                         timeout=120)
    pcm = np.frombuffer(res.stdout, dtype=np.int16)
    rf, au = sdr.design.mono_coeffs(151, 151)
    proc = sdr.MonoBlockProcessor(B, rf, au, iq_dtype=np.uint8)
    a = deemph(sdr, np.concatenate([proc.process(iq[2 * k * B:2 * (k + 1) * B]) for k in range(nb)]), 50e-6)
    assert pcm.shape == (nb * 2 * (B // 50),)
    accept(pcm, to_pcm(a, a))


@pytest.mark.gpu
def test_live_deemph_mode1_mono(sdr, gpu_ctx):
    nb = 3
    iq = sdr.synth.fm_iq(nb * B, seed=14, fs=2.5e6, dtype=np.uint8)
    res = subprocess.run([BIN, "--mode", "1", "--mono", "--deemph", "75"], input=iq.tobytes(), capture_output=True,
                         check=True, timeout=120)
    pcm = np.frombuffer(res.stdout, dtype=np.int16)
    A = (B // 10) * 24 // 125
    assert pcm.shape == (nb * 2 * A,)
    rf = signal.firwin(151, 100e3 / 1.25e6, window="hann")
    h = signal.firwin(3623, 16e3 / 3e6, window="hann")
    zi_i = zi_q = None
    ph, zr = 0.0, np.zeros(len(h) - 1)
    api = []
    for k in range(nb):
        d, zi_i, zi_q, ph = sdr.rf_frontend_block(iq[2 * k * B:2 * (k + 1) * B], rf, zi_i, zi_q, ph)
        y, zr = sdr.resample(d, h, zr, 24, 125)
        api.append(y[:A])
    a = deemph(sdr, np.concatenate(api), 75e-6)
    accept(pcm, to_pcm(a, a))
