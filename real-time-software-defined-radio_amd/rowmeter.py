"""Modulation meter of rows of real samples: what a modulation monitor shows of a demodulated FM
stream -- peak deviation, multiplex power, carrier offset, the share of samples beyond the limit, the
distribution of peak-hold values -- and of an audio row: peak, RMS, dead air.  Pure numpy; this
module is the definition the device stage (RowMeter, csrc/rmeter.hip) is tested against.

The rule, per stream, carried from call to call until reset (RowMeterModel):

  A sample is finite or not.  A non-finite sample counts in `nonfinite` and in nothing else.
  The call:   n (finite samples), nonfinite, over (finite samples with |x| > limit, a float32
              comparison), max and min (-inf / +inf without a finite sample), sum = sum float64(x),
              sumsq = sum float64(x)^2 (each square exact), windows (completed by this call).
  The totals: calls, total_n, total_nonfinite, total_over, total_max, total_min, total_sum,
              total_sumsq, total_windows, empty_windows.
  Windows:    the stream -- every sample, finite or not, counted by a 64-bit position -- is cut into
              consecutive windows of `window` samples, across calls.  A window keeps the max and min
              of its finite samples.  When it completes with at least one:
                  h   = float32(float32(max - min) * 0.5f)
                  bin = min(nbins - 1, floor(float32(h * scale)))
                  hist[bin] += 1                                       (uint64[nbins] per stream)
              one subtraction and two products in float32, none fused.  A window that completes
              without a finite sample counts in empty_windows only.  The unfinished window (wcount,
              wmax, wmin) is part of the state.
  windows():  the (min, max) pairs of the windows the latest call completed; (+inf, -inf) for one
              without a finite sample.

For a Receiver's "demod" rows (radians per sample at fs = 240 kS/s) x fs / 2 pi is the deviation in
Hz: modulation_report turns a record and a histogram into the monitor's figures.  mpx_levels reads
the pilot and RDS injection from RowSpectrum rows.
"""
from __future__ import annotations

import collections
import math

import numpy as np

from . import design

MIN_WINDOW, MAX_WINDOW, MAX_BINS, MAX_STREAMS = 64, 1 << 24, 1024, 4096
MAX_N = 2 ** 31 - 1
INT_FIELDS = ("n", "nonfinite", "over", "windows", "calls", "total_n", "total_nonfinite", "total_over", "total_windows",
              "empty_windows", "wcount")
F64_FIELDS = ("sum", "sumsq", "total_sum", "total_sumsq")
F32_FIELDS = ("max", "min", "total_max", "total_min", "wmax", "wmin")
# the order of include/sdr.h sdr_rmeter_record
FIELDS = ("n", "nonfinite", "over", "windows", "sum", "sumsq", "max", "min", "calls", "total_n", "total_nonfinite", "total_over",
          "total_windows", "empty_windows", "total_sum", "total_sumsq", "total_max", "total_min", "wcount", "wmax", "wmin")

RowMeterRecord = collections.namedtuple("RowMeterRecord", FIELDS)
RowMeterRecord.__doc__ = "The meter's state after a call: every field an array with one entry per stream (see the module text)."


def field_dtype(name):
    return np.int64 if name in INT_FIELDS else np.float64 if name in F64_FIELDS else np.float32


def check_params(nstreams, window, nbins, scale, limit):
    """The arguments of RowMeterModel and RowMeter as (nstreams, window, nbins, float32 scale, float32 limit);
    ValueError for what sdr_rmeter_create refuses."""
    nstreams, window, nbins = int(nstreams), int(window), int(nbins)
    if not 1 <= nstreams <= MAX_STREAMS:
        raise ValueError(f"nstreams={nstreams} outside [1, {MAX_STREAMS}]")
    if not MIN_WINDOW <= window <= MAX_WINDOW:
        raise ValueError(f"window={window} outside [{MIN_WINDOW}, 2^24]")
    if not 1 <= nbins <= MAX_BINS:
        raise ValueError(f"nbins={nbins} outside [1, {MAX_BINS}]")
    with np.errstate(over="ignore"):
        scale, limit = np.float32(scale), np.float32(limit)
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError(f"scale={scale} is not finite and positive")
    if np.isnan(limit):
        raise ValueError("limit is NaN")
    return nstreams, window, nbins, scale, limit


def as_rows(rows, nstreams):
    x = np.asarray(rows)
    if x.dtype != np.float32:
        x = x.astype(np.float32)
    if x.ndim == 1 and nstreams == 1:
        x = x[None, :]
    if x.ndim != 2 or x.shape[0] != nstreams or not 1 <= x.shape[1] <= MAX_N:
        raise ValueError(f"expected an array of shape ({nstreams}, n), 1 <= n <= 2^31 - 1")
    return x


def bins_of(wmax, wmin, scale, nbins):
    """The histogram bins of windows with the float32 peaks wmax >= wmin: the rule's three float32 steps."""
    with np.errstate(over="ignore"):
        h = (np.asarray(wmax, np.float32) - np.asarray(wmin, np.float32)) * np.float32(0.5)
        hb = (h * np.float32(scale)).astype(np.float32)
    b = np.full(hb.shape, nbins - 1, dtype=np.int64)
    inside = hb < np.float32(nbins)
    b[inside] = np.floor(hb[inside]).astype(np.int64)
    return b


class RowMeterModel:
    """The rule of the module text for `nstreams` rows: process(rows) takes one call of (nstreams, n)
    float32 samples; records(), hist() and windows() are what RowMeter's return."""

    def __init__(self, nstreams: int, window: int, nbins: int = 128, scale: float = 1.0, limit: float = np.inf):
        self.S, self.window, self.nbins, self.scale, self.limit = check_params(nstreams, window, nbins, scale, limit)
        self.reset()

    def reset(self):
        S = self.S
        self.pos = 0
        self._r = {k: np.zeros(S, dtype=field_dtype(k)) for k in FIELDS}
        for k in ("max", "total_max", "wmax"):
            self._r[k][:] = -np.inf
        for k in ("min", "total_min", "wmin"):
            self._r[k][:] = np.inf
        self._hist = np.zeros((S, self.nbins), dtype=np.uint64)
        self._win = np.zeros((S, 0, 2), dtype=np.float32)

    def process(self, rows):
        x = as_rows(rows, self.S)
        S, n, W, r = self.S, x.shape[1], self.window, self._r
        w0 = self.pos % W
        K, Kc = -(-(w0 + n) // W), (w0 + n) // W                    # windows the call touches, and completes
        starts = np.maximum(np.arange(K, dtype=np.int64) * W - w0, 0)
        win = np.empty((S, Kc, 2), dtype=np.float32)
        for s in range(S):
            row = x[s]
            fin = np.isfinite(row)
            v = row[fin]
            d = v.astype(np.float64)
            r["n"][s], r["nonfinite"][s] = v.size, n - v.size
            r["over"][s] = np.count_nonzero(np.abs(v) > self.limit)
            r["max"][s] = v.max() if v.size else -np.inf
            r["min"][s] = v.min() if v.size else np.inf
            r["sum"][s], r["sumsq"][s] = np.sum(d), np.sum(d * d)
            wmax = np.maximum.reduceat(np.where(fin, row, np.float32(-np.inf)), starts)
            wmin = np.minimum.reduceat(np.where(fin, row, np.float32(np.inf)), starts)
            wmax[0], wmin[0] = max(wmax[0], r["wmax"][s]), min(wmin[0], r["wmin"][s])
            done_max, done_min = wmax[:Kc], wmin[:Kc]
            some = done_max >= done_min
            np.add.at(self._hist[s], bins_of(done_max[some], done_min[some], self.scale, self.nbins), np.uint64(1))
            r["empty_windows"][s] += Kc - np.count_nonzero(some)
            win[s, :, 0], win[s, :, 1] = done_min, done_max
            r["wmax"][s], r["wmin"][s] = (wmax[Kc], wmin[Kc]) if K > Kc else (-np.inf, np.inf)
        r["windows"][:] = Kc
        r["wcount"][:] = (w0 + n) % W
        r["calls"] += 1
        for k in ("n", "nonfinite", "over", "windows", "sum", "sumsq"):
            r["total_" + k] += r[k]
        r["total_max"], r["total_min"] = np.maximum(r["total_max"], r["max"]), np.minimum(r["total_min"], r["min"])
        self.pos += n
        self._win = win
        return self

    def records(self) -> RowMeterRecord:
        return RowMeterRecord(*(self._r[k].copy() for k in FIELDS))

    def hist(self) -> np.ndarray:
        return self._hist.copy()

    def windows(self) -> np.ndarray:
        """float32[nstreams, windows, 2]: (min, max) of the windows the latest call completed."""
        return self._win.copy()


def row_meter_model(rows, window: int, nbins: int = 128, scale: float = 1.0, limit: float = np.inf):
    """One call of the rule on fresh state: (records, hist, windows) of rows (nstreams, n)."""
    x = np.asarray(rows, dtype=np.float32)
    x = x[None, :] if x.ndim == 1 else x
    m = RowMeterModel(x.shape[0], window, nbins, scale, limit).process(x)
    return m.records(), m.hist(), m.windows()


class ModulationReport(collections.namedtuple("ModulationReport", "carrier_offset_hz peak_pos_hz peak_neg_hz mpx_power_dbr "
                                              "mpx_power_dbr_call over_share windows hist bin_hz")):
    """modulation_report's figures, an array entry per stream; deviation_percentile reads the histogram."""
    __slots__ = ()

    def deviation_percentile(self, p: float) -> np.ndarray:
        """Per stream, the upper edge in Hz of the bin at which the cumulative count of window
        half-spans reaches p percent of the windows (0 < p <= 100); NaN without a binned window."""
        if not 0.0 < p <= 100.0:
            raise ValueError(f"p={p} outside (0, 100]")
        cum = np.cumsum(self.hist.astype(np.float64), axis=-1)
        total = cum[..., -1]
        first = np.argmax(cum >= (p * total[..., None]) / 100.0, axis=-1)
        return np.where(total > 0, (first + 1) * self.bin_hz, np.nan)


MPX_REF_HZ = 19e3                                 # 0 dBr: a sine of +-19 kHz peak deviation (ITU-R BS.412)


def _dbr(ssum, ssq, n, fs):
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = ssum / n
        var = ssq / n - mean * mean
        return 10.0 * np.log10(var * (fs / (2 * math.pi)) ** 2 / (MPX_REF_HZ ** 2 / 2))


def modulation_report(record: RowMeterRecord, hist, fs: float = design.AUDIO_FS, bin_hz: float = 1e3) -> ModulationReport:
    """A modulation monitor's figures from a meter's record and histogram (rows in radians per sample
    at fs, bins of bin_hz): carrier_offset_hz = total_sum / total_n fs / 2 pi; peak_pos_hz and
    peak_neg_hz from total_max and total_min; mpx_power_dbr = 10 log10(var (fs / 2 pi)^2 / (19e3^2 / 2))
    with var = total_sumsq / total_n - mean^2, and mpx_power_dbr_call the same of the latest call
    alone (what a caller keeps a 60 s sliding value of); over_share = total_over / total_n.  A
    stream without a finite sample reads NaN."""
    fs, k = float(fs), float(fs) / (2 * math.pi)
    n = np.asarray(record.total_n, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        offset = record.total_sum / n * k
        share = record.total_over / n
    peaks = [np.where(n > 0, np.asarray(v, np.float64) * k, np.nan) for v in (record.total_max, record.total_min)]
    return ModulationReport(offset, peaks[0], peaks[1], _dbr(record.total_sum, record.total_sumsq, n, fs),
                            _dbr(record.sum, record.sumsq, np.asarray(record.n, np.float64), fs), share,
                            np.asarray(record.total_windows), np.asarray(hist), float(bin_hz))


MpxLevels = collections.namedtuple("MpxLevels", "pilot_hz rds_hz")
PILOT_HZ, RDS_HZ, RDS_HALF_BAND_HZ, PILOT_HALF_BINS = 19e3, 57e3, 2.4e3, 2


def mpx_levels(power_rows, fs: float, nfft: int, window="hann") -> MpxLevels:
    """Pilot and RDS-subcarrier injection in Hz of deviation from RowSpectrum rows of a "demod" row
    (any shape (..., nfft / 2 + 1), linear power, bin k centred on k fs / nfft).  The power of a line
    is the sum of the bins it leaks into over the window's equivalent noise bandwidth in bins,
    nfft sum(w^2) / sum(w)^2; a sine of that power has the amplitude sqrt(2 P) radians per sample,
    times fs / 2 pi in Hz.  Pilot: the bins within +-2 of the one nearest 19 kHz.  RDS: the bins whose
    centres lie in 57 kHz +- 2.4 kHz, read as the sine of the same power."""
    p = np.asarray(power_rows, dtype=np.float64)
    nfft, fs = int(nfft), float(fs)
    if p.ndim < 1 or p.shape[-1] != nfft // 2 + 1:
        raise ValueError("power_rows: rows of nfft / 2 + 1 bins")
    if not fs / 2 > RDS_HZ + RDS_HALF_BAND_HZ:
        raise ValueError(f"fs={fs}: the RDS band needs fs / 2 above {RDS_HZ + RDS_HALF_BAND_HZ} Hz")
    w = design.spectrum_window(window, nfft)
    enbw = nfft * float(np.sum(w * w)) / float(np.sum(w)) ** 2
    f = np.arange(p.shape[-1]) * (fs / nfft)
    k0 = int(round(PILOT_HZ * nfft / fs))
    pilot = np.sum(p[..., k0 - PILOT_HALF_BINS:k0 + PILOT_HALF_BINS + 1], axis=-1) / enbw
    rds = np.sum(p[..., np.abs(f - RDS_HZ) <= RDS_HALF_BAND_HZ], axis=-1) / enbw
    return MpxLevels(np.sqrt(2.0 * pilot) * fs / (2 * math.pi), np.sqrt(2.0 * rds) * fs / (2 * math.pi))
