"""Capture ingest: the raw IQ formats wideband front ends write, as the float32 capture every stage
reads, and the level meter a user sets the front end's gain by.  Pure numpy; this module is the
definition the device stage (CaptureIngest, csrc/ingest.hip) is tested against.

A capture is 2 n interleaved values I0 Q0 I1 Q1 ... of one of four formats:

  cu8    uint8 (rtl_sdr)                        code c = x - 128, bits = 8
  cs8    int8 (HackRF .cs8, SigMF ci8)          code c = x, bits = 8
  cs16   native little-endian int16 (Airspy, SDRplay, bladeRF, LimeSDR, USRP .cs16; SigMF ci16_le)
         code c = x; `bits` (2..16, default 16) is the width of the right-justified, sign-extended
         ADC code in the word: 12 for a 12-bit ADC
  cf32   float32: passes through bit for bit, NaN and infinities included

out = float32(c * 2^-(bits - 1)), exact for every code; for cu8 it is the project's (x - 128) / 128.
swap=True exchanges I and Q in the output (a front end with an inverted spectrum).  The meter is
taken on the input and does not depend on swap.

The meter of a call, integer formats -- every field an integer and exact:
  n           samples
  clipped     samples whose I or Q code is >= 2^(bits - 1) - 1 or <= -2^(bits - 1); codes beyond a
              narrower `bits` count too
  peak_code   max |c| over I and Q (the most negative code counts with its magnitude)
  sumsq_code  sum of cI^2 + cQ^2, an unsigned 64-bit integer: n <= 2^31 - 1 samples of at most 2^31
              each stay below 2^62
  peak = peak_code 2^-(bits - 1) and sumsq = float64(sumsq_code) 2^-2(bits - 1); nonfinite = 0
cf32:
  nonfinite   samples with a non-finite I or Q; they are left out of everything else
  clipped     |I| >= 1 or |Q| >= 1
  peak        the largest |x|, exact
  sumsq       the float64 sum of the float64 squares (a product of two float32 values is exact)
  peak_code = sumsq_code = 0
Carried from call to call: calls, total_n, total_clipped.
"""
from __future__ import annotations

import collections
import math
import os

import numpy as np

# fmt -> (numpy dtype of a value, container width in bits)
FORMATS = {"cu8": (np.dtype(np.uint8), 8), "cs8": (np.dtype(np.int8), 8), "cs16": (np.dtype("<i2"), 16),
           "cf32": (np.dtype("<f4"), 32)}
_NAMES = {"cu8": "cu8", "cs8": "cs8", "cs16": "cs16", "cf32": "cf32",          # the formats and file extensions
          "ci8": "cs8", "ci16_le": "cs16", "cf32_le": "cf32"}                  # SigMF core:datatype
MAX_N = 2 ** 31 - 1


def capture_format(name) -> str:
    """A file name (extension .cu8 .cs8 .cs16 .cf32, any case) or a format name (those, or SigMF's
    cu8 ci8 ci16_le cf32_le) -> 'cu8' | 'cs8' | 'cs16' | 'cf32'; anything else raises ValueError."""
    if not isinstance(name, (str, os.PathLike)):
        raise ValueError(f"capture format {name!r}: a file name or a format name")
    text = os.fspath(name)
    ext = os.path.splitext(text)[1]
    if ext:
        fmt = ext[1:].lower()
        if fmt in FORMATS:
            return fmt
        raise ValueError(f"{text!r}: extension {ext} is none of .cu8 .cs8 .cs16 .cf32")
    if text.lower() in _NAMES:
        return _NAMES[text.lower()]
    raise ValueError(f"capture format {text!r}: one of {' '.join(_NAMES)}")


def check_format(fmt, bits=None):
    """(fmt, bits) of the arguments `fmt` (a format name, or numpy's uint8 / int8 / int16 / float32) and
    `bits` (None: the container's width; cs16: 2..16; refused for the others unless it is their width)."""
    if isinstance(fmt, str):
        if fmt not in FORMATS:
            raise ValueError(f"fmt {fmt!r}: one of {' '.join(FORMATS)}")
    else:
        try:
            dt = np.dtype(fmt)
        except TypeError:
            raise ValueError(f"fmt {fmt!r}: one of {' '.join(FORMATS)} or their numpy dtypes") from None
        match = [k for k, (d, _) in FORMATS.items() if d == dt]
        if not match:
            raise ValueError(f"fmt {dt}: uint8, int8, int16 or float32")
        fmt = match[0]
    width = FORMATS[fmt][1]
    if bits is None:
        return fmt, width
    if isinstance(bits, bool) or int(bits) != bits:
        raise ValueError(f"bits={bits!r}: an integer")
    bits = int(bits)
    if fmt == "cs16":
        if not 2 <= bits <= 16:
            raise ValueError(f"bits={bits} outside [2, 16]")
    elif bits != width:
        raise ValueError(f"bits={bits}: {fmt} is {width} bits wide")
    return fmt, bits


def as_raw(raw, fmt) -> np.ndarray:
    """A host capture as a 1-D contiguous array of 2 n interleaved values of the format's type: an array
    of that type, raw bytes (uint8) of any format, or complex64 for cf32."""
    dt = FORMATS[fmt][0]
    a = np.asarray(raw)
    if a.dtype != dt:
        if fmt == "cf32" and a.dtype == np.complex64:
            a = np.ascontiguousarray(a).view(dt)
        elif a.dtype == np.uint8 and a.ndim == 1 and a.nbytes % dt.itemsize == 0:
            a = np.ascontiguousarray(a).view(dt)
        else:
            raise ValueError(f"a {fmt} capture is {dt.name} values or raw bytes, not {a.dtype}")
    a = np.ascontiguousarray(a)
    if a.ndim != 1 or a.size % 2 or not 2 <= a.size <= 2 * MAX_N:
        raise ValueError("expected a 1-D array of 1 .. 2^31 - 1 interleaved I, Q pairs")
    return a


class IngestMeter(collections.namedtuple("IngestMeter", "n clipped nonfinite peak_code sumsq_code peak sumsq calls total_n total_clipped")):
    """The level meter after a call (see the module text), with the figures a gain setting needs."""
    __slots__ = ()

    @property
    def power_dbfs(self) -> float:
        """Mean power of the finite samples' I and Q values, dB relative to full scale; -inf for silence."""
        m = 2 * (self.n - self.nonfinite)
        return 10.0 * math.log10(self.sumsq / m) if m > 0 and self.sumsq > 0.0 else -math.inf

    @property
    def peak_dbfs(self) -> float:
        return 20.0 * math.log10(self.peak) if self.peak > 0.0 else -math.inf

    @property
    def clip_share(self) -> float:
        return self.clipped / self.n if self.n else 0.0


ZERO_METER = IngestMeter(0, 0, 0, 0, 0, 0.0, 0.0, 0, 0, 0)


def ingest_model(raw, fmt, bits=None, swap=False, prev=None):
    """The rule: (out, meter) of one call.  out is float32[2 n]; `prev`, the meter of the call before,
    carries calls, total_n and total_clipped (None: the first call after a reset)."""
    fmt, bits = check_format(fmt, bits)
    x = as_raw(raw, fmt)
    n = x.size // 2
    if fmt == "cf32":
        out = x.copy()
        a = np.abs(x.astype(np.float64))
        fin = np.isfinite(a[0::2]) & np.isfinite(a[1::2])
        m = np.maximum(a[0::2], a[1::2])[fin]
        v = x.astype(np.float64).reshape(n, 2)[fin]
        nonfinite, clipped = int(n - np.count_nonzero(fin)), int(np.count_nonzero(m >= 1.0))
        peak_code, sumsq_code = 0, 0
        peak, sumsq = (float(m.max()) if m.size else 0.0), float(np.sum(v * v))
    else:
        c = x.astype(np.int64) - (128 if fmt == "cu8" else 0)
        out = (c.astype(np.float64) * 2.0 ** -(bits - 1)).astype(np.float32)
        hi, lo = 2 ** (bits - 1) - 1, -2 ** (bits - 1)
        rail = (c >= hi) | (c <= lo)
        nonfinite, clipped = 0, int(np.count_nonzero(rail[0::2] | rail[1::2]))
        peak_code = int(np.max(np.abs(c)))
        sumsq_code = int(np.sum((c * c).astype(np.uint64), dtype=np.uint64))
        peak, sumsq = peak_code * 2.0 ** -(bits - 1), float(np.float64(np.uint64(sumsq_code))) * 2.0 ** (-2 * (bits - 1))
    if swap:
        out = np.ascontiguousarray(out.reshape(n, 2)[:, ::-1]).reshape(2 * n)
    prev = ZERO_METER if prev is None else prev
    return out, IngestMeter(n, clipped, nonfinite, peak_code, sumsq_code, peak, sumsq, prev.calls + 1, prev.total_n + n,
                            prev.total_clipped + clipped)
