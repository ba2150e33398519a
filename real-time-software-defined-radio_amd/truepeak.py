"""True peak of audio rows after ITU-R BS.1770-4 annex 2, and loudness range after EBU Tech 3342.
numpy; this module is the definition the device stage (TruePeakMeter, csrc/tpeak.hip) is tested
against, bit for bit.

The rule, per stream s, channel c and stream position t (input samples since reset, x[t] = 0 for
t < 0), with a table h float32 [L, P] (design.true_peak_fir(): L = 4 phases of P = 12 taps):

  y[t, p] = sum_{k = 0 .. P - 1} float64(h[p, k]) * float64(x[t - k])     float64, from 0.0, k ascending
            (a float32 x float32 product is exact in float64: a fused and an unfused multiply-add
            give the same bits)
  m[t]    = max |y[t, p]| over the finite y[t, p]; 0.0 if there is none
  q[t]    = |x[t]| if finite, else 0.0                                    the sample peak
  A non-finite y[t, p] counts in `nonfinite` (L per sample at most) and enters no maximum.

Segment g holds the positions with t // segment == g; its true peak is max m[t], its sample peak
max q[t].  The open segment's maxima, the position and the last P - 1 samples are carried from call
to call (TruePeakModel).  The record per (stream, channel) is include/sdr.h's sdr_tpeak_record: of
the latest call n (its samples), nonfinite, peak, sample_peak; since reset calls, total_n,
total_nonfinite, total_peak, total_sample_peak and segments (completed); open_peak and
open_sample_peak of the unfinished segment.

true_peak_report turns maxima into dBTP and dBFS relative to `reference`, the row amplitude of PCM
full scale (2.0: sosfilter.py).  loudness_range reads the segment energies of a LoudnessMeter.
"""
from __future__ import annotations

import collections

import numpy as np

from . import design
from .sosfilter import ABSOLUTE_GATE, OFFSET, as_rows, check_loudness_params

MAX_UP, MAX_TAPS = 8, 32                           # include/sdr.h SDR_TPEAK_MAX_UP, SDR_TPEAK_MAX_TAPS
LRA_RELATIVE_GATE, LRA_LOW, LRA_HIGH, LRA_SEGMENTS = -20.0, 0.10, 0.95, 30   # EBU Tech 3342: LU, percentiles, 3 s of 100 ms

INT_FIELDS = ("n", "nonfinite", "calls", "total_n", "total_nonfinite", "segments")
# the order of include/sdr.h sdr_tpeak_record
FIELDS = ("n", "nonfinite", "peak", "sample_peak", "calls", "total_n", "total_nonfinite", "total_peak", "total_sample_peak", "segments",
          "open_peak", "open_sample_peak")

TruePeakRecord = collections.namedtuple("TruePeakRecord", FIELDS)
TruePeakRecord.__doc__ = "A true-peak meter's state after a call: every field an array [nstreams, channels] (see the module text)."


def field_dtype(name):
    return np.int64 if name in INT_FIELDS else np.float64


def check_taps(taps) -> np.ndarray:
    """`taps` as float32 [L, P] (None: design.true_peak_fir()); ValueError for what sdr_tpeak_create refuses."""
    if taps is None:
        return design.true_peak_fir()
    with np.errstate(over="ignore"):
        h = np.array(taps, dtype=np.float32, ndmin=2)
    if h.ndim != 2:
        raise ValueError(f"taps must be [up, taps], not {h.shape}")
    if not 1 <= h.shape[0] <= MAX_UP:
        raise ValueError(f"up={h.shape[0]} outside [1, {MAX_UP}]")
    if not 1 <= h.shape[1] <= MAX_TAPS:
        raise ValueError(f"taps={h.shape[1]} outside [1, {MAX_TAPS}]")
    if not np.all(np.isfinite(h)):
        raise ValueError("taps has a non-finite coefficient")
    return np.ascontiguousarray(h)


def check_params(nstreams, channels, segment, cap, taps):
    """The arguments of TruePeakModel and TruePeakMeter as (nstreams, channels, segment, cap, float32 taps)."""
    nstreams, channels, segment, cap, _ = check_loudness_params(nstreams, channels, segment, cap, 1.0)
    return nstreams, channels, segment, cap, check_taps(taps)


class TruePeakModel:
    """The rule of TruePeakMeter (see the module text), with every completed segment kept.
    process(rows): a list of `channels` arrays [S, n]; peaks() and sample_peaks(): float64
    [S, channels, nseg]; records(): a TruePeakRecord."""

    def __init__(self, nstreams: int, channels: int, segment: int = 4800, taps=None):
        self.nstreams, self.channels, self.segment, _, self.taps = check_params(nstreams, channels, segment, 4, taps)
        self.reset()

    def reset(self):
        S, C = self.nstreams, self.channels
        self.pos = 0
        self.hist = np.zeros((S, C, self.taps.shape[1] - 1), dtype=np.float32)
        self._r = {k: np.zeros((S, C), dtype=field_dtype(k)) for k in FIELDS}
        self._pk, self._sp = [], []                                 # [S, C] per completed segment

    def process(self, rows):
        if len(rows) != self.channels:
            raise ValueError(f"{len(rows)} row sets for {self.channels} channels")
        xs = [as_rows(r, self.nstreams) for r in rows]
        n = xs[0].shape[1]
        if any(x.shape[1] != n for x in xs):
            raise ValueError("the channels' rows differ in length")
        L, P = self.taps.shape
        h = self.taps.astype(np.float64)
        x = np.concatenate([self.hist, np.stack(xs, axis=1)], axis=2)      # [S, C, P - 1 + n] float32
        xd = x.astype(np.float64)
        m = np.zeros((self.nstreams, self.channels, n))
        bad = np.zeros((self.nstreams, self.channels, n), dtype=np.int64)
        with np.errstate(invalid="ignore", over="ignore"):
            for p in range(L):
                y = np.zeros_like(m)
                for k in range(P):
                    y = y + h[p, k] * xd[:, :, P - 1 - k:P - 1 - k + n]
                fin = np.isfinite(y)
                m = np.maximum(m, np.where(fin, np.abs(y), 0.0))
                bad += ~fin
            own = x[:, :, P - 1:]
            q = np.where(np.isfinite(own), np.abs(own), np.float32(0.0)).astype(np.float64)
        r = self._r
        r["n"][:] = n
        r["nonfinite"][:] = np.sum(bad, axis=2)
        r["peak"][:], r["sample_peak"][:] = np.max(m, axis=2), np.max(q, axis=2)
        i = 0
        while i < n:
            take = min(n - i, self.segment - self.pos % self.segment)
            r["open_peak"] = np.maximum(r["open_peak"], np.max(m[:, :, i:i + take], axis=2))
            r["open_sample_peak"] = np.maximum(r["open_sample_peak"], np.max(q[:, :, i:i + take], axis=2))
            i += take
            self.pos += take
            if self.pos % self.segment == 0:
                self._pk.append(r["open_peak"])
                self._sp.append(r["open_sample_peak"])
                r["open_peak"], r["open_sample_peak"] = np.zeros_like(r["peak"]), np.zeros_like(r["peak"])
        r["calls"] += 1
        r["total_n"] += n
        r["total_nonfinite"] += r["nonfinite"]
        r["total_peak"], r["total_sample_peak"] = np.maximum(r["total_peak"], r["peak"]), np.maximum(r["total_sample_peak"], r["sample_peak"])
        r["segments"][:] = self.pos // self.segment
        self.hist = np.ascontiguousarray(x[:, :, n:])
        return self

    def _kept(self, done) -> np.ndarray:
        if not done:
            return np.zeros((self.nstreams, self.channels, 0))
        return np.ascontiguousarray(np.stack(done, axis=2))

    def peaks(self) -> np.ndarray:
        return self._kept(self._pk)

    def sample_peaks(self) -> np.ndarray:
        return self._kept(self._sp)

    def records(self) -> TruePeakRecord:
        return TruePeakRecord(*(self._r[k].copy() for k in FIELDS))


TruePeakReport = collections.namedtuple("TruePeakReport", "true_peak_dbtp sample_peak_dbfs total_true_peak_dbtp latest_dbtp nonfinite")
TruePeakReport.__doc__ = """true_peak_report's figures, an array entry per stream: true_peak_dbtp and sample_peak_dbfs over the kept
segments, total_true_peak_dbtp since the last reset, latest_dbtp of the last completed segment (-inf where
there is nothing to measure: no segment yet, silence), nonfinite (interpolated values left out since reset)."""


def _db(v, reference):
    with np.errstate(divide="ignore"):
        return 20.0 * np.log10(np.asarray(v, dtype=np.float64) / reference)


def true_peak_report(peaks, sample_peaks, records: TruePeakRecord, reference: float = 2.0) -> TruePeakReport:
    """A meter's figures from the kept segments [S, channels, nseg] (TruePeakModel.peaks() /
    sample_peaks(), TruePeakMeter.segments()) and its records, per stream over the channels:
    true_peak_dbtp = 20 log10(max / reference) and sample_peak_dbfs likewise over the kept segments,
    total_true_peak_dbtp from the records' running maximum since reset (not limited to the ring: it
    holds the open segment too), latest_dbtp from the last completed segment, nonfinite the values
    left out since reset.  `reference` is the row amplitude of PCM full scale."""
    pk, sp = np.asarray(peaks, dtype=np.float64), np.asarray(sample_peaks, dtype=np.float64)
    if pk.ndim != 3 or sp.shape != pk.shape:
        raise ValueError(f"peaks and sample_peaks must be [S, channels, nseg], not {pk.shape} and {sp.shape}")
    reference = float(reference)
    if not (np.isfinite(reference) and reference > 0):
        raise ValueError(f"reference={reference} is not finite and positive")
    S = pk.shape[0]
    over = lambda a: np.max(a.reshape(S, -1), axis=1) if a.size else np.zeros(S)   # noqa: E731
    return TruePeakReport(_db(over(pk), reference), _db(over(sp), reference), _db(np.max(records.total_peak, axis=1), reference),
                          _db(over(pk[:, :, -1:]), reference), np.sum(records.total_nonfinite, axis=1))


LoudnessRange = collections.namedtuple("LoudnessRange", "lra low high values gated")
LoudnessRange.__doc__ = """loudness_range's figures, an array entry per stream: lra in LU (0.0 with fewer than two gated values),
low and high (the 10th and 95th percentile in LUFS; NaN where lra is 0.0 for want of values), values (the
finite short-term values; the max(nseg - 29, 0) - values others were left out) and gated (those that passed
both gates)."""


def loudness_range(energies, segment: int, fs: float = 48e3) -> LoudnessRange:
    """EBU Tech 3342 loudness range from segment energies [S, channels, nseg] (LoudnessModel.energies(),
    LoudnessMeter.segments()) of 100 ms segments: the short-term loudness -0.691 + 10 log10(sum_ch mean
    square) of every run of 30 consecutive segments (3 s, a hop of one segment); the values at or
    below -70 LUFS are dropped, then those at or below the loudness of the mean power of the rest
    - 20 LU; of what is left, sorted ascending as v, lra = v[round((len - 1) 0.95)] -
    v[round((len - 1) 0.10)].  Non-finite values are left out (and counted: see LoudnessRange)."""
    e = np.asarray(energies, dtype=np.float64)
    if e.ndim != 3:
        raise ValueError(f"energies must be [S, channels, nseg], not {e.shape}")
    segment = int(segment)
    if segment < 1 or abs(segment * 10 - fs) > 1e-6 * fs:
        raise ValueError(f"segment={segment} is not 100 ms at fs={fs}")
    S, _, nseg = e.shape
    tot = np.sum(e, axis=1)
    nst = max(nseg - LRA_SEGMENTS + 1, 0)
    lra, low, high = np.zeros(S), np.full(S, np.nan), np.full(S, np.nan)
    values, gated = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
    for s in range(S):
        ms = np.array([np.sum(tot[s, i:i + LRA_SEGMENTS]) for i in range(nst)]) / (LRA_SEGMENTS * float(segment))
        ms = ms[np.isfinite(ms)]
        values[s] = ms.size
        with np.errstate(divide="ignore"):
            ms = ms[OFFSET + 10.0 * np.log10(ms) > ABSOLUTE_GATE]
            if ms.size:
                ms = ms[OFFSET + 10.0 * np.log10(ms) > OFFSET + 10.0 * np.log10(np.mean(ms)) + LRA_RELATIVE_GATE]
        gated[s] = ms.size
        if ms.size >= 2:
            v = np.sort(OFFSET + 10.0 * np.log10(ms))
            low[s], high[s] = v[int(np.floor((v.size - 1) * LRA_LOW + 0.5))], v[int(np.floor((v.size - 1) * LRA_HIGH + 0.5))]
            lra[s] = high[s] - low[s]
    return LoudnessRange(lra, low, high, values, gated)
