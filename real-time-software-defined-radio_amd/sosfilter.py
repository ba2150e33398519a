"""Cascades of second-order sections on rows of real samples, and programme loudness after ITU-R
BS.1770 built on them.  numpy / scipy; this module is the definition the device stages (RowSos,
LoudnessMeter, csrc/sos.hip) are tested against.

  sos_model        scipy.signal.sosfilt per row in float64, rounded once to float32; the state is
                   scipy's zi / zf (direct form II transposed), [K, 2] per row.
  LoudnessModel    every row through the two K-weighting sections (design.k_weighting_sos) with
                   carried state, scaled by 1 / `reference` (one float64 product a sample), and the
                   float64 sum of squares of every completed segment of `segment` samples of stream
                   position.  The squares are of the float64 filter output: no row rounded to float32
                   is in the path.
  loudness_report  the energies of 100 ms segments as momentary, short-term and gated integrated
                   loudness in LUFS.

`reference` is the row amplitude that stands for PCM full scale.  The receiver's output stage writes
int16(x * 16384) (include/sdr.h sdr_audio_out_dev), so int16 full scale, 32768, is the row amplitude
32768 / 16384 = 2.0: a sine of amplitude 2.0 on an audio row is a 0 dBFS sine, and BS.1770's 997 Hz
full-scale sine in one channel reads -3.01 LUFS.
"""
from __future__ import annotations

import collections

import numpy as np
from scipy import signal

from . import design

MAX_SECTIONS, MAX_ROWS = 4, 4096                   # include/sdr.h SDR_SOS_MAX_SECTIONS, SDR_SOS_MAX_ROWS
MIN_SEGMENT, MAX_SEGMENT, MAX_CAP = 2048, 1 << 24, 1 << 20
MAX_N = 2 ** 31 - 1
ABSOLUTE_GATE, RELATIVE_GATE, OFFSET = -70.0, -10.0, -0.691   # BS.1770-4 5.1: LUFS, LU, the 997 Hz calibration


def check_sos(sos) -> np.ndarray:
    """`sos` as float64 [K, 6]; ValueError for what sdr_sos_create refuses."""
    sos = np.array(sos, dtype=np.float64, ndmin=2)
    if sos.ndim != 2 or sos.shape[1] != 6:
        raise ValueError(f"sos must be [K, 6], not {sos.shape}")
    K = sos.shape[0]
    if not 1 <= K <= MAX_SECTIONS:
        raise ValueError(f"K={K} outside [1, {MAX_SECTIONS}]")
    if not np.all(np.isfinite(sos)):
        raise ValueError("sos has a non-finite coefficient")
    for k, s in enumerate(sos):
        if s[3] != 1.0:
            raise ValueError(f"a0={s[3]} of section {k} is not 1")
        if abs(s[5]) >= 1.0 or abs(s[4]) >= 1.0 + s[5]:
            raise ValueError(f"section {k} (a1={s[4]}, a2={s[5]}) has a pole on or outside the unit circle")
    return np.ascontiguousarray(sos)


def check_rows_count(nrows, noun="nrows") -> int:
    nrows = int(nrows)
    if not 1 <= nrows <= MAX_ROWS:
        raise ValueError(f"{noun}={nrows} outside [1, {MAX_ROWS}]")
    return nrows


def as_rows(rows, nrows) -> np.ndarray:
    x = np.asarray(rows)
    if x.dtype != np.float32:
        x = x.astype(np.float32)
    if x.ndim == 1 and nrows == 1:
        x = x[None, :]
    if x.ndim != 2 or x.shape[0] != nrows or x.shape[1] < 1:
        raise ValueError(f"rows must be ({nrows}, n >= 1), not {x.shape}")
    return x


def sos_model(sos, x_rows, zi=None):
    """(y float32 [S, n], zf float64 [S, K, 2]): scipy.signal.sosfilt(sos, float64(x), zi=zi) per row,
    rounded once.  zi: [S, K, 2] (None: zeros)."""
    sos = check_sos(sos)
    x = np.asarray(x_rows)
    x = (x[None, :] if x.ndim == 1 else x).astype(np.float64)
    S, K = x.shape[0], sos.shape[0]
    z = np.zeros((S, K, 2)) if zi is None else np.array(zi, dtype=np.float64).reshape(S, K, 2)
    y, zf = signal.sosfilt(sos, x, axis=-1, zi=np.ascontiguousarray(z.transpose(1, 0, 2)))
    return y.astype(np.float32), np.ascontiguousarray(zf.transpose(1, 0, 2))


def check_loudness_params(nstreams, channels, segment, cap, reference):
    nstreams, channels, segment, cap, reference = check_rows_count(nstreams, "nstreams"), int(channels), int(segment), int(cap), float(reference)
    if channels not in (1, 2):
        raise ValueError(f"channels={channels} is not 1 or 2")
    if not MIN_SEGMENT <= segment <= MAX_SEGMENT:
        raise ValueError(f"segment={segment} outside [{MIN_SEGMENT}, 2^24]")
    if not 4 <= cap <= MAX_CAP:
        raise ValueError(f"cap={cap} outside [4, 2^20]")
    if not (np.isfinite(reference) and reference > 0):
        raise ValueError(f"reference={reference} is not finite and positive")
    return nstreams, channels, segment, cap, reference


class LoudnessModel:
    """The rule of LoudnessMeter (see the module text), with every completed segment kept.
    process(rows): a list of `channels` arrays [S, n]; energies(): float64 [S, channels, nseg]."""

    def __init__(self, nstreams: int, channels: int, segment: int = 4800, reference: float = 2.0):
        self.nstreams, self.channels, self.segment, _, self.reference = check_loudness_params(nstreams, channels, segment, 4, reference)
        self.sos = design.k_weighting_sos()
        self.reset()

    def reset(self):
        self.zi = np.zeros((self.channels, self.nstreams, 2, 2))
        self.pos = 0
        self.open = np.zeros((self.nstreams, self.channels))
        self.done = []                                              # [S, channels] per completed segment

    def process(self, rows):
        if len(rows) != self.channels:
            raise ValueError(f"{len(rows)} row sets for {self.channels} channels")
        xs = [as_rows(r, self.nstreams) for r in rows]
        n = xs[0].shape[1]
        w = np.empty((self.nstreams, self.channels, n))
        for ch, x in enumerate(xs):
            if x.shape[1] != n:
                raise ValueError("the channels' rows differ in length")
            y, zf = signal.sosfilt(self.sos, x.astype(np.float64), axis=-1, zi=np.ascontiguousarray(self.zi[ch].transpose(1, 0, 2)))
            self.zi[ch] = zf.transpose(1, 0, 2)
            w[:, ch] = y * (1.0 / self.reference)
        i = 0
        while i < n:
            take = min(n - i, self.segment - self.pos % self.segment)
            self.open = self.open + np.sum(w[:, :, i:i + take] ** 2, axis=2)
            i += take
            self.pos += take
            if self.pos % self.segment == 0:
                self.done.append(self.open)
                self.open = np.zeros((self.nstreams, self.channels))
        return self

    def energies(self) -> np.ndarray:
        if not self.done:
            return np.zeros((self.nstreams, self.channels, 0))
        return np.ascontiguousarray(np.stack(self.done, axis=2))


LoudnessReport = collections.namedtuple("LoudnessReport", "momentary short_term integrated blocks gated_blocks nonfinite_blocks")
LoudnessReport.__doc__ = """loudness_report's figures, an array entry per stream: momentary, short_term and integrated in LUFS
(-inf where there is nothing to measure: no block yet, silence, no block above the absolute gate),
blocks (gating blocks in the energies), gated_blocks (those that passed both gates), nonfinite_blocks."""


def _lufs(ms):
    with np.errstate(divide="ignore"):
        return OFFSET + 10.0 * np.log10(ms)


def loudness_report(energies, segment: int, fs: float = 48e3) -> LoudnessReport:
    """BS.1770-4 loudness from segment energies [S, channels, nseg] (LoudnessModel.energies(),
    LoudnessMeter.segments()): the sums of squares of K-weighted samples over consecutive segments of
    `segment` samples, which must be 100 ms (fs / 10).  A gating block is 4 consecutive segments
    (400 ms, 75 % overlap), its loudness l = -0.691 + 10 log10(sum_ch mean square), channel weights
    1.  momentary: the latest block.  short_term: the latest 30 segments (3 s).  integrated: the
    blocks above -70 LUFS, then of those the ones above their mean's loudness - 10 LU; the loudness
    of the mean of what is left.  Blocks with a non-finite sum are left out and counted."""
    e = np.asarray(energies, dtype=np.float64)
    if e.ndim != 3:
        raise ValueError(f"energies must be [S, channels, nseg], not {e.shape}")
    segment = int(segment)
    if segment < 1 or abs(segment * 10 - fs) > 1e-6 * fs:
        raise ValueError(f"segment={segment} is not 100 ms at fs={fs}")
    S, _, nseg = e.shape
    tot = np.sum(e, axis=1)                                         # [S, nseg]
    mom, st, integ = np.full(S, -np.inf), np.full(S, -np.inf), np.full(S, -np.inf)
    nblk = max(nseg - 3, 0)
    gated, nonfinite = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
    if nblk:
        blk = (tot[:, 0:nblk] + tot[:, 1:nblk + 1] + tot[:, 2:nblk + 2] + tot[:, 3:nblk + 3]) / (4.0 * segment)   # mean squares [S, nblk]
        for s in range(S):
            ok = np.isfinite(blk[s])
            nonfinite[s] = nblk - np.count_nonzero(ok)
            if ok[-1]:
                mom[s] = _lufs(blk[s, -1])
            z = blk[s, ok]
            z = z[_lufs(z) > ABSOLUTE_GATE]
            if z.size:
                z = z[_lufs(z) > _lufs(np.mean(z)) + RELATIVE_GATE]
            gated[s] = z.size
            if z.size:
                integ[s] = _lufs(np.mean(z))
    if nseg >= 30:
        ms = np.sum(tot[:, nseg - 30:], axis=1) / (30.0 * segment)
        st = np.where(np.isfinite(ms), _lufs(np.where(np.isfinite(ms), ms, 0.0)), -np.inf)
    return LoudnessReport(mom, st, integ, np.full(S, nblk, dtype=np.int64), gated, nonfinite)
