"""Filter-coefficient design (host side, once per configuration).

The reference designs taps on the host too -- ``scipy.signal.firwin`` in the Python
model (model/fmMonoBlock.py:43,45,115,150,159; model/fmRDSblock.py:64-111) and
``impulseResponseLPF/BPF/RRC`` in the C++ (src/filter.cpp:19-93), the latter
recomputed every block (src/fm_radio.cpp:75).  Taps are data to the kernels; this
module only produces them.  Constants follow model/fmMonoBlock.py:22-32 and
model/fmRDSblock.py:24-47.
"""
from __future__ import annotations

import math

import numpy as np
from scipy import signal

# model/fmMonoBlock.py:22-32
RF_FS = 2.4e6
RF_FC = 100e3
RF_TAPS = 151
RF_DECIM = 10
AUDIO_FS = 240e3
AUDIO_FC = 16e3
AUDIO_TAPS = 151
AUDIO_DECIM = 5

# model/fmRDSblock.py:38-47, 94-111
RDS_BPF = (54000.0, 60000.0)
RDS_SQ_BPF = (113500.0, 114500.0)
RDS_PLL_FREQ = 114000.0
RDS_PHASE_ADJ = math.pi / 3.3 - math.pi / 1.5
RDS_PLL_BW = 0.001
RDS_PLL_SCALE = 0.5
RDS_LPF_FC = 3000.0
RDS_UP, RDS_DOWN = 19, 80
RRC_FS = 57000.0
RRC_TAPS = 151

# stereo (model/fmMonoBlock.py:115-162)
PILOT_BPF = (18.5e3, 19.5e3)
STEREO_BPF = (22e3, 54e3)
PILOT_FREQ = 19e3
STEREO_PLL_SCALE = 2.0


def deemphasis_coeffs(tau: float = 75e-6, fs: float = 48e3):
    """(b, a) of the FM de-emphasis filter: the bilinear transform of 1 / (1 + s tau), prewarped
    so that the -3 dB point stays at 1 / (2 pi tau) -- scipy.signal.bilinear([wca], [1, wca], fs)
    with wca = 2 fs tan(1 / (2 fs tau)).  tau: 75e-6 (Americas, Korea) or 50e-6 (elsewhere).
    The reference has no de-emphasis; this is the filter broadcast receivers apply to undo the
    transmitter's pre-emphasis."""
    if not (tau > 0 and fs > 0):
        raise ValueError("tau and fs must be positive")
    wca = 2.0 * fs * math.tan(1.0 / (2.0 * fs * tau))
    k = wca / (2.0 * fs)
    return np.array([k / (1.0 + k), k / (1.0 + k)]), np.array([1.0, -(1.0 - k) / (1.0 + k)])


def channel_coeffs(decim: int, taps=None) -> np.ndarray:
    """The channelizer's low-pass (Channelizer, sdr_ddc): signal.firwin(taps or 8 * decim,
    1.0 / decim) -- the cutoff at the output Nyquist; the receiver's own RF filter does the
    selective work.  decim 1 decimates nothing and needs no filter: a unit impulse."""
    decim = int(decim)
    if decim < 1:
        raise ValueError("decim must be >= 1")
    taps = int(taps) if taps else 8 * decim
    if decim == 1:
        return np.eye(1, taps)[0]
    return signal.firwin(taps, 1.0 / decim)


def pfb_coeffs(nbins: int, taps_per_bin: int = 8) -> np.ndarray:
    """The filter bank's prototype low-pass (FilterBank, sdr_pfb): signal.firwin(nbins *
    taps_per_bin, 1.0 / nbins) -- the cutoff at half the bin spacing, in Nyquist units.  One bin
    is the whole band and needs no filter: a unit impulse."""
    nbins, taps_per_bin = int(nbins), int(taps_per_bin)
    if nbins < 1 or taps_per_bin < 1:
        raise ValueError("nbins and taps_per_bin must be >= 1")
    if nbins == 1:
        return np.eye(1, taps_per_bin)[0]
    return signal.firwin(nbins * taps_per_bin, 1.0 / nbins)


def resample_coeffs(up: int, down: int, taps=None) -> np.ndarray:
    """The row resampler's low-pass (RowResampler, sdr_rsmp), designed at `up` times the input
    rate: signal.firwin(T, 1 / max(up, down), window=('kaiser', 5.0)) with T = taps or
    min(20 max(up, down) + 1, 4096) -- scipy.signal.resample_poly's default filter (unit DC gain;
    the resampler applies the gain `up`), cut to the library's longest filter."""
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise ValueError("up and down must be >= 1")
    big = max(up, down)
    taps = int(taps) if taps else min(20 * big + 1, 4096)
    if taps < 1:
        raise ValueError("taps must be >= 1")
    return signal.firwin(taps, 1.0 / big, window=("kaiser", 5.0))


def ddc_phase_inc(nu: float) -> int:
    """The channelizer's phase increment for a frequency of nu cycles per sample
    (|nu| <= 0.5): rint(nu 2^32) mod 2^32, as a Python int in [0, 2^32)."""
    nu = float(nu)
    if not (math.isfinite(nu) and abs(nu) <= 0.5):
        raise ValueError(f"frequency {nu} cycles/sample is not a finite value in [-0.5, 0.5]")
    return int(np.rint(nu * 4294967296.0)) % (1 << 32)


def ddc_actual_freq(inc: int) -> float:
    """The frequency a phase increment stands for, cycles per sample: signed(inc) / 2^32."""
    inc = int(inc) % (1 << 32)
    return (inc - (1 << 32) if inc >= (1 << 31) else inc) / 4294967296.0


def firwin_lpf(taps: int, fc: float, fs: float) -> np.ndarray:
    """signal.firwin(taps, fc/(fs/2), window='hann') as at model/fmMonoBlock.py:43."""
    return signal.firwin(taps, fc / (fs / 2), window=("hann"))


def firwin_bpf(taps: int, f_lo: float, f_hi: float, fs: float) -> np.ndarray:
    """signal.firwin(..., pass_zero='bandpass') as at model/fmMonoBlock.py:115."""
    return signal.firwin(taps, [f_lo / (fs / 2), f_hi / (fs / 2)], window=("hann"), pass_zero="bandpass")


def my_filterImpulseResponse(Fc, Fs, N_taps) -> np.ndarray:
    """Windowed sinc with a sin^2 window (model/fmSupportLib.py:144-154)."""
    fc = Fc / (Fs / 2)
    i = np.arange(N_taps, dtype=np.float64)
    off = i - (N_taps - 1) / 2
    arg = np.pi * fc * off
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(off == 0, fc, fc * np.sin(arg) / arg)
    return sinc * np.sin(np.pi * i / N_taps) ** 2


def impulseResponseRootRaisedCosine(Fs, N_taps) -> np.ndarray:
    """Root-raised-cosine taps, roll-off 0.90 at 2375 symbols/s (model/fmRRC.py:12-47).

    Same three cases as the reference: t == 0, |t| == Ts/(4 beta) (exact float
    comparison), and the general closed form; 1/Ts scale ignored as there.
    """
    ts, beta = 1 / 2375.0, 0.90
    t = (np.arange(N_taps, dtype=np.float64) - N_taps / 2) / Fs
    x = 4 * beta * t / ts
    with np.errstate(invalid="ignore", divide="ignore"):
        general = (np.sin(np.pi * t * (1 - beta) / ts) + x * np.cos(np.pi * t * (1 + beta) / ts)) / \
                  (np.pi * t * (1 - x * x) / ts)
    at_zero = 1.0 + beta * (4 / np.pi - 1)
    q = np.pi / (4 * beta)
    at_edge = beta / np.sqrt(2) * ((1 + 2 / np.pi) * np.sin(q) + (1 - 2 / np.pi) * np.cos(q))
    edge = (t == ts / (4 * beta)) | (t == -ts / (4 * beta))
    return np.where(t == 0.0, at_zero, np.where(edge, at_edge, general))


def mono_coeffs(rf_taps: int = RF_TAPS, audio_taps: int = AUDIO_TAPS):
    """(rf_coeff, audio_coeff) exactly as model/fmMonoBlock.py:43-45."""
    return firwin_lpf(rf_taps, RF_FC, RF_FS), firwin_lpf(audio_taps, AUDIO_FC, AUDIO_FS)


def stereo_coeffs(taps: int = RF_TAPS):
    """(pilot BPF, stereo-band BPF, stereo LPF), model/fmMonoBlock.py:115,150,159."""
    return (firwin_bpf(taps, *PILOT_BPF, AUDIO_FS),
            firwin_bpf(taps, *STEREO_BPF, AUDIO_FS),
            firwin_lpf(taps, 16e3, AUDIO_FS))


def rds_coeffs(taps: int = RF_TAPS):
    """RDS filters of model/fmRDSblock.py:88-111 (extract, squared BPF, 3k LPF, anti-image, RRC)."""
    return dict(
        extract=firwin_bpf(taps, *RDS_BPF, AUDIO_FS),
        square=firwin_bpf(taps, *RDS_SQ_BPF, AUDIO_FS),
        lpf=firwin_lpf(taps, RDS_LPF_FC, AUDIO_FS),
        anti_img=signal.firwin(taps, (57000 / 2) / ((240000 * 19) / 2), window=("hann")),
        rrc=impulseResponseRootRaisedCosine(RRC_FS, RRC_TAPS),
    )


def spectrum_window(window, nfft: int) -> np.ndarray:
    """The nfft window values of a Spectrum (f64): a name (or tuple) for
    scipy.signal.get_window(window, nfft) -- the periodic form, as scipy.signal.spectrogram
    uses -- or an array of nfft finite values of any sign whose sum is not zero."""
    if isinstance(window, (str, tuple)):
        w = signal.get_window(window, int(nfft))
    else:
        w = np.atleast_1d(np.asarray(window))
        if w.ndim != 1 or len(w) != nfft or np.iscomplexobj(w):
            raise ValueError(f"{w.shape} window values: nfft={nfft} real ones")
    w = np.ascontiguousarray(w, dtype=np.float64)
    if not np.all(np.isfinite(w)):
        raise ValueError("window values must be finite")
    if np.sum(w) == 0.0:
        raise ValueError("the window sums to zero")
    return w


def k_weighting_sos(fs: float = 48e3) -> np.ndarray:
    """The two K-weighting sections of ITU-R BS.1770-4 (tables 1 and 2) as sos [2, 6]: the
    pre-filter (a high shelf for the head's acoustics) and the RLB high-pass.  The standard
    tabulates 48 kHz only, and the receiver's audio rows are 48 kHz: any other rate is refused."""
    if fs != 48e3:
        raise ValueError(f"K-weighting is tabulated at 48 kHz only, not fs={fs}")
    return np.array([[1.53512485958697, -2.69169618940638, 1.19839281085285, 1.0, -1.69065929318241, 0.73248077421585],
                     [1.0, -2.0, 1.0, 1.0, -1.99004745483398, 0.99007225036621]])


TRUE_PEAK_FIR_8192 = ((14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68),
                      (-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155))


def true_peak_fir() -> np.ndarray:
    """The 48-tap, 4-phase interpolator of ITU-R BS.1770-4 annex 2 (x4 oversampling of 48 kHz rows) as
    float32 [4, 12]: integers / 8192, each exact in float32; phases 2 and 3 are phases 1 and 0
    reversed.  Phase p, tap k weighs the sample k in front of the newest."""
    a = np.array(TRUE_PEAK_FIR_8192, dtype=np.float64)
    return np.ascontiguousarray(np.concatenate([a, a[::-1, ::-1]]) / 8192.0, dtype=np.float32)


def pilot_notch_sos(fs: float = 48e3, f0: float = PILOT_FREQ, q: float = 30.0) -> np.ndarray:
    """A notch at the 19 kHz pilot for the audio rows: signal.tf2sos(*signal.iirnotch(f0, q, fs)),
    one section, -3 dB width f0 / q."""
    return signal.tf2sos(*signal.iirnotch(f0, q, fs))
