"""The synthetic wideband capture of the IQ-correction tests (tests/test_iqc_model.py on the CPU,
tests/test_iqc.py on the GPU) and the image measure.

Signal: fs = 19.2 MHz; stations at +3.1, -5.3, +0.9, -7.7 MHz with amplitudes 1, 0.5, 0.3, 0.2, each
FM-modulated to 75 kHz deviation by white noise low-passed to about 15 kHz (peak-normalised), plus
complex white noise of sigma 0.003 per branch; the sum scaled by 0.3.
Impairment: I = I0 + 0.03, Q = 1.06 (Q0 cos 4deg + I0 sin 4deg) - 0.02; |I|, |Q| <= 0.65, so the uint8
form (round(128 x) + 128) does not clip.
Image measure: Hann-windowed FFT of the block; the power within +-120 kHz of -f over the power
within +-120 kHz of +f, in dB."""
import functools

import numpy as np

FS = 19.2e6
STATIONS = ((3.1e6, 1.0), (-5.3e6, 0.5), (0.9e6, 0.3), (-7.7e6, 0.2))
DEVIATION, AUDIO_BW, NOISE_SIGMA, SCALE = 75e3, 15e3, 0.003, 0.3
GAIN, PHASE_DEG, DC = 1.06, 4.0, (0.03, -0.02)
C1 = -np.tan(np.deg2rad(PHASE_DEG))                    # what the estimate should find
C2 = 1.0 / (GAIN * np.cos(np.deg2rad(PHASE_DEG)))
IMAGE_HALF_WIDTH = 120e3


def _audio(rng, n):
    """white noise low-passed to about AUDIO_BW (a brick wall in the FFT), peak 1"""
    spec = np.fft.rfft(rng.standard_normal(n))
    spec[np.fft.rfftfreq(n, 1.0 / FS) > AUDIO_BW] = 0.0
    a = np.fft.irfft(spec, n)
    return a / np.max(np.abs(a))


@functools.lru_cache(maxsize=None)
def _ideal(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    z = np.zeros(n, dtype=np.complex128)
    for f, amp in STATIONS:
        phase = 2.0 * np.pi * DEVIATION * np.cumsum(_audio(rng, n)) / FS
        z += amp * np.exp(1j * (2.0 * np.pi * f * t + phase + rng.uniform(0.0, 2.0 * np.pi)))
    z += NOISE_SIGMA * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    z *= SCALE
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def _capture(n, seed, impaired, u8):
    z = _ideal(n, seed)
    i, q = z.real, z.imag
    if impaired:
        th = np.deg2rad(PHASE_DEG)
        i, q = i + DC[0], GAIN * (z.imag * np.cos(th) + z.real * np.sin(th)) + DC[1]
    x = np.empty(2 * n)
    x[0::2], x[1::2] = i, q
    assert np.max(np.abs(x)) < 127.0 / 128.0                   # the uint8 form does not clip
    out = (np.rint(128.0 * x) + 128.0).astype(np.uint8) if u8 else x.astype(np.float32)
    out.setflags(write=False)
    return out


def capture(n, dtype=np.float32, seed=0, impaired=True):
    """A read-only interleaved capture of n complex samples, float32 or uint8 (cached)."""
    return _capture(int(n), int(seed), bool(impaired), np.dtype(dtype) == np.uint8)


def as_complex(iq):
    """interleaved float32 or uint8 -> complex128"""
    x = np.asarray(iq).astype(np.float64)
    if np.asarray(iq).dtype == np.uint8:
        x = (x - 128.0) / 128.0
    return x[0::2] + 1j * x[1::2]


def image_db(iq, f):
    """10 log10 of the power around -f over the power around +f of an interleaved block."""
    z = as_complex(iq)
    n = len(z)
    p = np.abs(np.fft.fft(z * np.hanning(n))) ** 2
    fr = np.fft.fftfreq(n, 1.0 / FS)
    at = lambda c: float(np.sum(p[np.abs(fr - c) <= IMAGE_HALF_WIDTH]))   # noqa: E731
    return 10.0 * np.log10(at(-f) / at(f))
