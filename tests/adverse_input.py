"""Adverse FM captures for the span tests: synth.fm_iq's composite (same amplitudes: 0.45 (L+R)/2,
a 0.1 pilot, 0.45 (L-R)/2 on twice the pilot's angle, 0.05 x random +-1 symbols on three times it)
with a pilot that is offset, buried in in-band noise, or switched off and back with a phase jump --
the inputs on which a PLL does NOT lock in its first pseudo-block and stay locked
(tests/test_compact_rows.py checks that they stay adverse, on the CPU).

The impairments go into the composite, not the IQ: the FM demodulator stays as well conditioned
as on the clean capture, so every row upstream of the loops keeps its tolerance."""
import numpy as np

FS = 2.4e6
SYM = 1010                     # samples per RDS symbol

# name -> adverse_iq's keyword arguments (the RDS band's noise as the pilot's)
CASES = {
    "J": dict(pilot_offset_hz=7.0, pilot_noise=0.3, rds_noise=0.3),
    "S": dict(pilot_offset_hz=40.0, pilot_noise=0.8, rds_noise=0.8),
    "U": dict(pilot_offset_hz=2.0, pilot_noise=1.5, rds_noise=1.5),
    # the pilot (and the subcarriers derived from it) off for 30 000 IQ samples in the second
    # pseudo-block of each K = 3 span (3 x 153 600 IQ samples), back 2.6 rad later
    "D": dict(gaps=((170_000, 200_000), (630_800, 660_800)), jump=2.6),
}


def _band_noise(rng, n, lo, hi, std):
    """white noise masked by FFT to [lo, hi] Hz, scaled to the standard deviation std"""
    if std == 0:
        return np.zeros(n)
    spec = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1.0 / FS)
    spec[(f < lo) | (f > hi)] = 0.0
    x = np.fft.irfft(spec, n)
    return x * (std / np.std(x))


def adverse_iq(n_complex, seed, pilot_offset_hz=0, pilot_noise=0, rds_noise=0, gaps=(), jump=0.0):
    """Interleaved u8 IQ of n_complex samples.
    pilot_noise / rds_noise: in-band noise (17-21 kHz / 54-60 kHz) of standard deviation
    pilot_noise x 0.1 / rds_noise x 0.05 (the pilot's / the RDS subcarrier's amplitude);
    gaps: (a, b) in IQ samples -- pilot and both subcarriers zero in [a, b), the pilot's phase
    advanced by `jump` rad after each."""
    import rtsdr
    rng = np.random.default_rng(seed)
    n = int(n_complex)
    t = np.arange(n, dtype=np.float64) / FS
    left = np.sin(2 * np.pi * 1e3 * t)
    right = 0.8 * np.sin(2 * np.pi * 2.5e3 * t)
    sym = rng.choice(np.array([-1.0, 1.0]), size=n // SYM + 1)[np.arange(n) // SYM]
    on = np.ones(n)
    phi = np.zeros(n)
    for a, b in gaps:
        on[a:b] = 0.0
        phi[b:] += jump
    theta = 2 * np.pi * (19e3 + pilot_offset_hz) * t + phi
    mpx = 0.45 * (left + right) / 2 + on * (0.1 * np.cos(theta) + 0.45 * (left - right) / 2 * np.cos(2 * theta)
                                            + 0.05 * sym * np.cos(3 * theta))
    mpx += _band_noise(rng, n, 17e3, 21e3, pilot_noise * 0.1)
    mpx += _band_noise(rng, n, 54e3, 60e3, rds_noise * 0.05)
    ph = 2 * np.pi * 75e3 * np.cumsum(mpx) / FS
    amp = 0.5
    sigma = amp / np.sqrt(2.0) * 10 ** (-30.0 / 20.0)
    noise = rng.standard_normal((n, 2)) * sigma
    iq = np.empty(2 * n, dtype=np.float32)
    iq[0::2] = amp * np.cos(ph) + noise[:, 0]
    iq[1::2] = amp * np.sin(ph) + noise[:, 1]
    u8 = rtsdr.synth.to_u8(iq)
    # no exact-zero sample (I = Q = 128 is 0 / 0 in the demodulator)
    zero = (u8[0::2] == 128) & (u8[1::2] == 128)
    u8[0::2][zero] = 129
    return u8
