"""Device-resident block pipelines: the loops of model/fmMonoBlock.py and
model/fmRDSblock.py with every intermediate and every carried state in HBM.

All of them run on libsdr's multi-stream block receiver (sdr_rx_*, csrc/rx.hip): one
block of S independent streams is a fixed chain of ~10 launches -- the RF front end, one
launch per filter stage for all of that stage's filters and their lfilter final states,
and one lane per PLL recurrence -- whatever S is.  Per block only the IQ goes
host->device and the requested outputs come back; filter states (lfilter zi, f64), demod
phases and PLL states never leave the GPU.  Stage order and state threading follow the
reference loops:

  Receiver              S streams of any of the below at once
  MonoBlockProcessor    model/fmMonoBlock.py:86-109   
  StereoBlockProcessor  model/fmMonoBlock.py:113-173  (a9, a10; intended combiner)
  RdsBlockProcessor     model/fmRDSblock.py:133-204   (a9, a11; up to the RRC output)
"""
from __future__ import annotations

import collections
import contextlib
import ctypes

import numpy as np

from . import _lib
from . import capture
from . import design
from . import iqbalance
from . import rowmeter
from . import sosfilter
from . import truepeak
from ._lib import RX_FILTERS, RX_OUTPUTS, SDR_IQ_F32, SDR_IQ_U8, SDR_RX_AUDIO, SDR_RX_RDS, SDR_RX_STEREO, check, f64p
from .dsp import _taps

_PLL_INIT = (0.0, 0.0, 1.0, 0.0, 1.0, 0.0)       # model/fmMonoBlock.py:76, model/fmRDSblock.py:96


def _addr(a):
    """The data address of a C-contiguous array: a writable one through the buffer protocol
    (~0.6 us), anything else through ndarray.ctypes (~1.5-2 us, a ctypes object per call).
    At the reference's block sizes a block costs ~30-45 us, so per-call pointer lookups show."""
    if a.flags.writeable and a.nbytes:
        return ctypes.addressof(ctypes.c_char.from_buffer(a))
    return a.ctypes.data


class _Handle:
    """A libsdr object: `lib`, its `handle` (None until created, and again once closed, so that
    __del__ is safe after a failed constructor) and the C prefix of its functions."""

    _prefix = None
    handle = None

    def _do(self, op, *args):
        name = f"{self._prefix}_{op}"
        check(getattr(self.lib, name)(self.handle, *args), name)

    def close(self):
        if self.handle:
            getattr(self.lib, f"{self._prefix}_destroy")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _LazyHandle(_Handle):
    """A libsdr object made at the first call that needs it: the constructor checks its arguments
    without a context and keeps `ctx` in _ctx (None: the default context); _create_args() gives
    what <prefix>_create takes between the context and the handle."""

    _ctx = None

    def _open(self):
        if self.handle is None:
            self.ctx = self._ctx if self._ctx is not None else _lib.get_context()
            self.lib = self.ctx.lib
            h, name = ctypes.c_void_p(), f"{self._prefix}_create"
            check(getattr(self.lib, name)(self.ctx.handle, *self._create_args(), ctypes.byref(h)), name)
            self.handle = h
        return self.handle

    def _do(self, op, *args):
        self._open()
        super()._do(op, *args)

    def _ptr_out(self, op, count=1):
        """The device pointer <prefix>_<op> hands out (count > 1: a tuple of them)."""
        p = [ctypes.c_void_p() for _ in range(count)]
        self._do(op, *(ctypes.byref(q) for q in p))
        return p[0].value if count == 1 else tuple(q.value for q in p)


class _Timed:
    """HIP events between the launches of each call, for an object whose C prefix has _set_timing
    and _stage_ms: _STAGES names the launches."""

    _STAGES = ()

    def set_timing(self, on: bool = True):
        """Record HIP events between the object's launches (stage_ms); off in measured loops."""
        self._do("set_timing", int(bool(on)))

    def stage_ms(self) -> dict:
        """GPU milliseconds per launch of the last timed call (set_timing(True) first), by _STAGES."""
        ms = (ctypes.c_float * len(self._STAGES))()
        self._do("stage_ms", ms)
        return dict(zip(self._STAGES, (float(v) for v in ms)))


def _check_capture_call(name, ptr, es, n, out_ptr, in_place_ok, owner):
    """The call rule of a pass over a capture block (CaptureIngest, IqCorrector): n complex samples
    of es bytes at device pointer `<name>_ptr` to n complex float32 at out_ptr, which may be the
    same pointer where in_place_ok (`owner` says for whom).  Returns (ptr, n, out_ptr) as ints."""
    n, ptr, out_ptr = int(n), int(ptr or 0), int(out_ptr or 0)
    if not ptr or not out_ptr:
        raise ValueError(f"{name}_ptr or out_ptr is NULL")
    if not 1 <= n <= capture.MAX_N:
        raise ValueError(f"n={n} outside [1, 2^31 - 1]")
    if ptr % es or out_ptr % 8:
        raise ValueError(f"{name}_ptr must be aligned to one complex sample ({es} B) and out_ptr to 8 B")
    if ptr < out_ptr + 8 * n and out_ptr < ptr + es * n and not (in_place_ok and ptr == out_ptr):
        raise ValueError(f"{name} and out overlap (only out_ptr == {name}_ptr of {owner} may)")
    return ptr, n, out_ptr


class _Stream(_Handle):
    """A block that carries a history and a stream position from call to call."""

    @property
    def position(self) -> int:
        """Input samples taken since the last reset (plus its position, where it takes one)."""
        p = ctypes.c_int64()
        self._do("position", ctypes.byref(p))
        return p.value

    def reset(self):
        """Zero the history of every row; the position back to 0."""
        self._do("reset")


class _DecimBlock(_Stream):
    """One interleaved-IQ capture to `nch` rows at fs / decim (Channelizer, FilterBank): the
    call rules and the two entry points."""

    _noun = None

    def reset(self, position: int = 0):
        """Zero the filter history and set the stream position (>= 0, a multiple of decim)."""
        self._do("reset", int(position))

    def _check_n(self, n, out_stride=None):
        if n < 1 or n % self.decim:
            raise ValueError(f"n={n} must be >= 1 and a multiple of decim={self.decim}")
        if out_stride is not None and out_stride < n // self.decim:
            raise ValueError(f"out_stride={out_stride} < n/decim={n // self.decim}")

    def process(self, iq) -> np.ndarray:
        """n complex samples from the host (interleaved f32 / u8, or complex for an f32
        object) -> (nch, n / decim) complex64, synchronous (sdr_ddc_run / sdr_pfb_run)."""
        iq = _interleaved_iq(iq, self.u8, self._noun)
        n = iq.size // 2
        self._check_n(n)
        out = np.empty((self.nch, n // self.decim), dtype=np.complex64)
        self._do("run", iq.ctypes.data, n, out.ctypes.data, n // self.decim)
        return out

    def process_dev(self, iq_ptr: int, n: int, out_ptr: int, out_stride: int):
        """n complex samples at device pointer iq_ptr -> rows of n / decim complex f32 at
        out_ptr, out_stride complex samples apart; async on the context stream."""
        n, out_stride = int(n), int(out_stride)
        self._check_n(n, out_stride)
        self._do("process_dev", iq_ptr, n, out_ptr, out_stride)


def _interleaved_iq(iq, u8, noun):
    """A host capture as a 1-D array of interleaved I, Q values of the object's type."""
    iq = np.asarray(iq)
    if np.iscomplexobj(iq):
        if u8:
            raise ValueError(f"a uint8 {noun} takes interleaved uint8 IQ")
        iq = np.ascontiguousarray(iq, dtype=np.complex64).view(np.float32)
    iq = np.ascontiguousarray(iq, dtype=np.uint8 if u8 else np.float32)
    if iq.ndim != 1 or iq.size % 2:
        raise ValueError("expected a 1-D array of interleaved I, Q values")
    return iq


def _real_taps(taps, max_taps, designed, count_checked=True):
    """A `taps` argument -- an array of real taps, a tap count or None -- as 1 .. max_taps finite
    float64 taps; designed(count or None) makes the last two."""
    if taps is None or np.ndim(taps) == 0:
        if count_checked and taps is not None and not 1 <= int(taps) <= max_taps:
            raise ValueError(f"taps={taps} outside [1, {max_taps}]")
        taps = designed(taps)
    b = np.ascontiguousarray(np.atleast_1d(np.asarray(taps)), dtype=np.float64)
    if b.ndim != 1 or not 1 <= len(b) <= max_taps:
        raise ValueError(f"{b.shape} taps: 1..{max_taps} real taps")
    if not np.all(np.isfinite(b)):
        raise ValueError("taps must be finite")
    return b


def _is_u8(iq_dtype):
    """An `iq_dtype` argument: float32 (False) or uint8 (True)."""
    dt = np.dtype(iq_dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.uint8)):
        raise ValueError(f"iq_dtype {dt}: float32 or uint8")
    return dt == np.uint8


class Receiver(_Timed, _Handle):
    """`nstreams` independent FM streams through the block receiver (sdr_rx).

    Each call to process() takes one block of every stream: an (nstreams, 2*block) array of
    interleaved IQ (f32, or u8 as read from rtl_sdr, src/iofunc.cpp:61-69).  mono=True
    produces the mono audio (model/fmMonoBlock.py:86-109); stereo=True adds the pilot PLL,
    the stereo channel and L/R (:113-173); rds=True the RDS chain to the RRC output
    (model/fmRDSblock.py:156-204).  Outputs (output(), process()'s return) are float32
    arrays of shape (nstreams, n); names as in the reference loops ("audio", "stereo",
    "left", "right", "rrc_i", ...: _lib.RX_OUTPUTS).

    deemphasis: an FM de-emphasis time constant in seconds (75e-6 or 50e-6; default None: off).
    The receiver then also produces "audio_de" ("left_de", "right_de" with stereo=True) -- the
    audio rows through design.deemphasis_coeffs(deemphasis, 240 kHz / audio_decim) on the device
    (sdr_rx_set_deemph), state carried from block to block -- and pcm(), the block's interleaved
    int16 samples; process()'s default outputs include the de-emphasised rows.

    blend: True (BlendParams' defaults) or a BlendParams (default False: off).  Needs deemphasis.
    Every block's "demod" rows then go through a RowSpectrum (blend_nfft, hop blend_nfft / 2,
    navg 0) and a BlendControl on the device, and the audio output stage ramps "left_de" /
    "right_de" and pcm() to the resulting stereo and mute gains (sdr_rx_set_blend; without stereo
    "audio_de" takes the mute gain; a stereo receiver's "audio_de" stays unblended).
    blend_state() reads the quality and gains back."""

    _prefix = "sdr_rx"
    _STAGES = _lib.RX_STAGES                                     # stage_ms: the stages of the last block

    def __init__(self, nstreams: int, block_complex: int, *, mono: bool = True, stereo: bool = False,
                 rds: bool = False, iq_dtype=np.uint8, rf_coeff=None, audio_coeff=None, stereo_taps: int = 151,
                 rds_taps: int = 151, rf_decim: int = 10, audio_decim: int = 5, pipeline: bool = False,
                 depth: int = 1, keep=None, deemphasis=None, blend=False, blend_nfft: int = 1024, ctx=None):
        # blend: its arguments are checked before a context exists
        self.blend = None if blend is False or blend is None else _blend_params(blend)
        self.blend_nfft = int(blend_nfft)
        if self.blend is not None:
            if deemphasis is None or not (mono or stereo):
                raise ValueError("blend needs the audio output stage: an audio output and deemphasis=tau")
            if not 512 <= self.blend_nfft <= Spectrum.MAX_NFFT or self.blend_nfft & (self.blend_nfft - 1):
                raise ValueError(f"blend_nfft={self.blend_nfft} must be a power of two in [512, {Spectrum.MAX_NFFT}]")
            if -(-int(block_complex) // int(rf_decim)) < self.blend_nfft:
                raise ValueError(f"blend_nfft={self.blend_nfft} exceeds the block's demod samples")
        self.ctx = ctx if ctx is not None else _lib.get_context()
        self.lib = self.ctx.lib
        self.S, self.B = int(nstreams), int(block_complex)
        self.u8 = np.dtype(iq_dtype) == np.uint8
        flags = (SDR_RX_AUDIO if mono else 0) | (SDR_RX_STEREO if stereo else 0) | (SDR_RX_RDS if rds else 0)
        self.flags = flags
        self._lengths = {}
        self._plans = {}
        self._pending = collections.deque()   # submit(): the blocks in flight's output arrays
        self.depth = int(depth)
        h = ctypes.c_void_p()
        check(self.lib.sdr_rx_create(self.ctx.handle, self.S, self.B, SDR_IQ_U8 if self.u8 else SDR_IQ_F32,
                                     flags, ctypes.byref(h)), "sdr_rx_create")
        self.handle = h
        if pipeline:                          # front half of block k+1 beside the back half of k
            check(self.lib.sdr_rx_set_pipeline(self.handle, 1), "sdr_rx_set_pipeline")
        if self.depth != 1:                   # submit(): `depth` blocks in flight
            check(self.lib.sdr_rx_set_depth(self.handle, self.depth), "sdr_rx_set_depth")
        if rf_coeff is None or audio_coeff is None:
            rc, ac = design.mono_coeffs()
            rf_coeff = rc if rf_coeff is None else rf_coeff
            audio_coeff = ac if audio_coeff is None else audio_coeff
        taps = {"rf": rf_coeff, "audio": audio_coeff}
        if stereo:
            taps.update(zip(("pilot", "stereo_bpf", "stereo_lpf"), design.stereo_coeffs(stereo_taps)))
        if rds:
            co = design.rds_coeffs(rds_taps)
            taps.update(rds_extract=co["extract"], rds_square=co["square"], rds_lpf=co["lpf"],
                        rds_anti=co["anti_img"], rds_rrc=co["rrc"])
        for name, b in taps.items():
            b = _taps(b)
            check(self.lib.sdr_rx_set_filter(self.handle, RX_FILTERS.index(name), f64p(b), len(b)),
                  "sdr_rx_set_filter")
        check(self.lib.sdr_rx_set_decim(self.handle, int(rf_decim), int(audio_decim), design.RDS_UP,
                                        design.RDS_DOWN), "sdr_rx_set_decim")
        self.deemphasis = None if deemphasis is None else float(deemphasis)
        if self.deemphasis is not None:
            if not flags & (SDR_RX_AUDIO | SDR_RX_STEREO):
                raise ValueError("deemphasis needs an audio output (mono=True or stereo=True)")
            b, a = design.deemphasis_coeffs(self.deemphasis, design.AUDIO_FS / audio_decim)
            self.deemph_coeffs = (b, a)
            check(self.lib.sdr_rx_set_deemph(self.handle, f64p(np.ascontiguousarray(b)), float(a[1])),
                  "sdr_rx_set_deemph")
        if self.blend is not None:
            check(self.lib.sdr_rx_set_blend(self.handle, ctypes.byref(self.blend._c()), self.blend_nfft), "sdr_rx_set_blend")
        if keep is not None:
            self.set_keep(keep)
        self.M = (self.B + rf_decim - 1) // rf_decim
        self.A = (self.M + audio_decim - 1) // audio_decim
        self.R = (self.M * design.RDS_UP + design.RDS_DOWN - 1) // design.RDS_DOWN

    @property
    def outputs(self):
        """Names of the outputs this configuration produces."""
        return [n for k, n in enumerate(RX_OUTPUTS) if self._produces(k)]

    def _produces(self, k):
        # mirrors the `group` and `deemph` columns of kOutput (csrc/rx_layout.h), which the library
        # answers from only once the receiver is finalised; tests/test_receiver.py holds the two together
        name = RX_OUTPUTS[k]
        if name == "demod":
            return True
        if name == "audio":
            return bool(self.flags & (SDR_RX_AUDIO | SDR_RX_STEREO))
        if name == "audio_de":
            return self.deemphasis is not None and bool(self.flags & (SDR_RX_AUDIO | SDR_RX_STEREO))
        if name in ("left_de", "right_de"):
            return self.deemphasis is not None and bool(self.flags & SDR_RX_STEREO)
        if k <= RX_OUTPUTS.index("right"):
            return bool(self.flags & SDR_RX_STEREO)
        return bool(self.flags & SDR_RX_RDS)

    def _call(self, fn, iq, fetch):
        es = np.uint8 if self.u8 else np.float32
        iq = np.ascontiguousarray(iq, dtype=es)
        if iq.size != self.S * 2 * self.B:
            raise ValueError(f"expected {self.S} x {2 * self.B} interleaved values, got {iq.shape}")
        key = tuple(fetch) if fetch is not None else None
        plan = self._plans.get(key)
        if plan is None:                      # output names -> (which[], lengths, offsets), built once
            names = list(fetch) if fetch is not None else \
                [n for n in ("audio", "left", "right", "rrc_i", "rrc_q", "audio_de", "left_de", "right_de")
                 if n in self.outputs]
            which = (ctypes.c_int * len(names))(*[RX_OUTPUTS.index(n) for n in names])
            lengths = [self._length(n) for n in names]
            offs = [self.S * sum(lengths[:i]) for i in range(len(names))]
            plan = self._plans[key] = (names, which, lengths, offs, self.S * sum(lengths),
                                       ctypes.c_void_p * len(names))
        names, which, lengths, offs, total, ptr_array = plan
        # one allocation per call, the outputs (S, n) views of it
        buf = np.empty(max(total, 1), dtype=np.float32)
        base = _addr(buf)
        ptrs = ptr_array(*[base + 4 * o for o in offs])
        outs = {n: buf[o:o + self.S * m].reshape(self.S, m) for n, o, m in zip(names, offs, lengths)}
        check(getattr(self.lib, fn)(self.handle, _addr(iq), self.B, len(names), which, ptrs, None), fn)
        return outs

    def process(self, iq, fetch=None):
        """One block of every stream; returns {name: (nstreams, n) float32} for `fetch`
        (default: the configuration's final outputs).  One C call: IQ up, the chain, the
        outputs down, one wait (sdr_rx_run)."""
        if self._pending:                     # submitted blocks are delivered (and dropped) first
            self.flush()
        return self._call("sdr_rx_run", iq, fetch)

    def submit(self, iq, fetch=None):
        """process() without waiting (sdr_rx_submit): launches this block and returns the
        outputs of the block submitted `depth` calls earlier (None while the pipeline fills:
        depth 1 = the PREVIOUS block), so the host prepares the next block while these run.
        flush() returns the rest."""
        self._pending.append(self._call("sdr_rx_submit", iq, fetch))
        return self._pending.popleft() if len(self._pending) > self.depth else None

    def flush(self):
        """Wait for every submitted block; returns the list of the blocks' outputs not yet
        returned by submit(), oldest first (empty when none is in flight), at any depth."""
        check(self.lib.sdr_rx_flush(self.handle), "sdr_rx_flush")
        rest = list(self._pending)
        self._pending.clear()
        return rest

    def _length(self, name):
        if name not in self._lengths:
            self._lengths[name] = self.output_ptr(name)[2]
        return self._lengths[name]

    def set_keep(self, names):
        """Outputs process_dev materialises (sdr_rx_set_keep; default: all).  Leaving out the
        NCO rows ("nco", "nco_i", "nco_q") and the RDS LPF rows ("lpf_i", "lpf_q") -- which the
        chain itself does not need -- keeps them out of HBM: the mixers form the NCO from the PLL
        phases and the RDS LPF runs inside the composite resampler (the same values either way).
        process() / submit() materialise what they are asked for."""
        mask = 0
        for n in names:
            mask |= 1 << RX_OUTPUTS.index(n)
        check(self.lib.sdr_rx_set_keep(self.handle, mask), "sdr_rx_set_keep")

    def process_dev(self, iq_ptr: int, iq_stride: int):
        """One block from device memory (async on the context stream); outputs stay on the
        GPU (output_ptr).  What is enqueued on the context stream before the next process_dev call
        (a stage's process_rx) sees this block's rows, also behind a pipelined receiver that the
        host runs blocks ahead of; later work must be waited for before the row set comes round."""
        check(self.lib.sdr_rx_process_dev(self.handle, iq_ptr, int(iq_stride)), "sdr_rx_process_dev")

    def output_ptr(self, name: str):
        """(device pointer, row stride in floats, samples per row) of output `name`."""
        p, st, n = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
        check(self.lib.sdr_rx_output(self.handle, RX_OUTPUTS.index(name), ctypes.byref(p), ctypes.byref(st),
                                     ctypes.byref(n)), "sdr_rx_output")
        return p.value, st.value, n.value

    def output(self, name: str) -> np.ndarray:
        _, _, n = self.output_ptr(name)
        out = np.empty((self.S, n), dtype=np.float32)
        check(self.lib.sdr_rx_fetch(self.handle, RX_OUTPUTS.index(name), out.ctypes.data_as(_lib._fp), n),
              "sdr_rx_fetch")
        return out

    def pcm(self) -> np.ndarray:
        """The latest block's interleaved int16 PCM (sdr_rx_pcm), shape (nstreams, 2 A): L0 R0 L1 R1 ..
        from "left_de" / "right_de" with stereo=True, else "audio_de" on both channels.  Needs
        deemphasis."""
        p, st, n = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
        check(self.lib.sdr_rx_pcm(self.handle, ctypes.byref(p), ctypes.byref(st), ctypes.byref(n)), "sdr_rx_pcm")
        buf = np.empty((self.S, st.value), dtype=np.int16)
        check(self.lib.sdr_memcpy_d2h(self.ctx.handle, buf.ctypes.data, p.value, buf.nbytes), "sdr_memcpy_d2h")
        return np.ascontiguousarray(buf[:, :n.value])

    def blend_state(self) -> "BlendState":
        """The blend's quality of the latest block and the gains its audio ramped to
        (sdr_rx_blend_state; synchronises): BlendControl.state().  Needs blend."""
        if self.blend is None:
            raise ValueError("blend_state needs a receiver with blend=True")
        raw = np.empty((self.S, BlendControl.NSTATE))
        check(self.lib.sdr_rx_blend_state(self.handle, f64p(raw)), "sdr_rx_blend_state")
        return _blend_state(raw)

    def state(self):
        """Carried states: (demod prev_phase [S], stereo PLL [S, 6], RDS PLL [S, 6])."""
        ph = np.empty(self.S)
        ps, pr = np.empty((self.S, 6)), np.empty((self.S, 6))
        check(self.lib.sdr_rx_state(self.handle, f64p(ph), f64p(ps), f64p(pr)), "sdr_rx_state")
        return ph, ps, pr

    def pll_stats(self, reset: bool = False) -> dict:
        """How the PLL recurrences were solved (sdr_rx_pll_stats: the context's counters, after
        every block in flight): counts by solver; see _lib.PLL_STATS."""
        return _lib.decode_pll_stats(lambda a: self.lib.sdr_rx_pll_stats(self.handle, a.ctypes.data,
                                                                         int(bool(reset))))

    def reset(self):
        check(self.lib.sdr_rx_reset(self.handle), "sdr_rx_reset")
        self._pending.clear()

    def rds_link(self, **kw) -> "RdsLinkBank":
        """A device-side RDS link layer sized to this receiver (RdsLinkBank: one stream per
        receiver stream, rows of the "rrc_i" length); feed it with bank.process_rx(receiver)
        after each block.  Needs rds=True."""
        if not self.flags & SDR_RX_RDS:
            raise ValueError("rds_link needs a receiver with rds=True")
        kw.setdefault("ctx", self.ctx)
        return RdsLinkBank(self.S, self._length("rrc_i"), **kw)

    def rds_clock(self, **kw) -> "RdsClockBank":
        """A device-side RDS symbol clock sized to this receiver (RdsClockBank: one stream per
        receiver stream, rows of the "rrc_i" length); feed it with bank.process_rx(receiver) after
        each block, and its bits into bank.block_sync() with bank.feed(sync).  Needs rds=True."""
        if not self.flags & SDR_RX_RDS:
            raise ValueError("rds_clock needs a receiver with rds=True")
        kw.setdefault("ctx", self.ctx)
        return RdsClockBank(self.S, self._length("rrc_i"), **kw)

    def rds_carrier(self, **kw) -> "RdsCarrierBank":
        """A device-side RDS carrier phase stage sized to this receiver (RdsCarrierBank: one stream
        per receiver stream, rows of the "rrc_i" length); per block carrier.process_rx(receiver),
        then carrier.feed(clock) with clock = carrier.clock().  Needs rds=True."""
        if not self.flags & SDR_RX_RDS:
            raise ValueError("rds_carrier needs a receiver with rds=True")
        kw.setdefault("ctx", self.ctx)
        return RdsCarrierBank(self.S, self._length("rrc_i"), **kw)

    def mpx_spectrum(self, nfft: int = 1024, hop=None, navg: int = 0, **kw) -> "RowSpectrum":
        """A RowSpectrum sized to this receiver's "demod" rows (one row per stream, the multiplex at
        design.AUDIO_FS; hop defaults to nfft / 2); feed it with spectrum.process_rx(receiver,
        out_ptr) after a block and read the rows with mpx_quality."""
        kw.setdefault("ctx", self.ctx)
        nfft = int(nfft)
        return RowSpectrum(self.S, nfft, design.AUDIO_FS, hop=nfft // 2 if hop is None else hop, navg=navg, **kw)

    def modulation_meter(self, window_s: float = 0.05, bin_hz: float = 1e3, limit_hz: float = 75e3, nbins: int = 128, **kw) -> "RowMeter":
        """A RowMeter sized to this receiver's "demod" rows (radians per sample at design.AUDIO_FS):
        windows of round(window_s AUDIO_FS) samples, histogram bins of bin_hz of peak deviation
        (scale = float32(AUDIO_FS / (2 pi bin_hz))), over-deviation beyond limit_hz (limit =
        float32(2 pi limit_hz / AUDIO_FS)).  Feed it with meter.process_rx(receiver) after a block and
        read meter.records() with modulation_report."""
        kw.setdefault("ctx", self.ctx)
        fs = design.AUDIO_FS
        return RowMeter(self.S, int(round(window_s * fs)), nbins=nbins, scale=np.float32(fs / (2 * np.pi * bin_hz)),
                        limit=np.float32(2 * np.pi * limit_hz / fs), **kw)

    def audio_meter(self, name: str = "audio", window_s: float = 0.05, scale: float = 128.0, limit: float = 1.0, nbins: int = 128, **kw) -> "RowMeter":
        """The same object on an audio row (`name`: "audio", "left", "right" or their _de forms):
        windows of round(window_s x the row's rate) samples, `scale` bins per unit of amplitude; peak,
        RMS (from sum and sumsq) and dead air (windows in bin 0) per stream.  Feed it with
        meter.process_rx(receiver, name)."""
        kw.setdefault("ctx", self.ctx)
        fs = design.AUDIO_FS * self._length(name) / self._length("demod")
        return RowMeter(self.S, int(round(window_s * fs)), nbins=nbins, scale=scale, limit=limit, **kw)


    def audio_filter(self, sos, **kw) -> "RowSos":
        """A RowSos (a cascade of second-order sections: design.pilot_notch_sos, an elliptic low-pass,
        a DC blocker) sized to this receiver, one row per stream; per block
        filt.process_rx(receiver, name) filters the rows of output `name` in place, or into out_ptr."""
        kw.setdefault("ctx", self.ctx)
        return RowSos(self.S, sos, **kw)

    def loudness_meter(self, **kw) -> "LoudnessMeter":
        """A LoudnessMeter sized to this receiver's 48 kHz audio rows: two channels on "left_de" /
        "right_de" with stereo=True, else one on "audio_de"; "left" / "right" / "audio" where the
        receiver has no de-emphasis.  Feed it with meter.process_rx(receiver) after a block and read
        meter.report()."""
        kw.setdefault("ctx", self.ctx)
        return LoudnessMeter(self.S, channels=len(self.loudness_rows()), **kw)

    def true_peak_meter(self, **kw) -> "TruePeakMeter":
        """A TruePeakMeter sized to this receiver's 48 kHz audio rows, the channels of loudness_meter():
        feed it with meter.process_rx(receiver) after a block and read meter.report()."""
        kw.setdefault("ctx", self.ctx)
        return TruePeakMeter(self.S, channels=len(self.loudness_rows()), **kw)

    def loudness_rows(self) -> tuple:
        """The outputs a loudness meter of this receiver reads (LoudnessMeter.process_rx's default)."""
        names = ("left", "right") if self.flags & SDR_RX_STEREO else ("audio",)
        return tuple(n + "_de" for n in names) if self._produces(RX_OUTPUTS.index(names[0] + "_de")) else names


class MonoBlockProcessor:
    """FE (RF LPF + decimate + atan2 demod) and mono audio LPF + decimate per block.

    block_complex: complex samples per block (model/fmMonoBlock.py:53 uses 51 200)."""

    _mode = dict(mono=True)

    def __init__(self, block_complex: int, rf_coeff=None, audio_coeff=None, rf_decim: int = 10,
                 audio_decim: int = 5, iq_dtype=np.float32, ctx=None, **kw):
        self.B = int(block_complex)
        self.rx = Receiver(1, self.B, iq_dtype=iq_dtype, rf_coeff=rf_coeff, audio_coeff=audio_coeff,
                           rf_decim=rf_decim, audio_decim=audio_decim, ctx=ctx, **self._mode, **kw)
        self.ctx = self.rx.ctx
        self.M, self.A = self.rx.M, self.rx.A

    def _run(self, iq_block, names):
        iq = np.asarray(iq_block)
        if iq.shape != (2 * self.B,):
            raise ValueError(f"expected {2 * self.B} interleaved values, got {iq.shape}")
        o = self.rx.process(iq, fetch=names)
        return {k: v[0].astype(np.float64) for k, v in o.items()}

    def process(self, iq_block, return_demod: bool = False):
        """audio_block (float64) for one block [+ fm_demod]; with deemphasis=tau, the
        de-emphasised audio block."""
        au = "audio" if self.rx.deemphasis is None else "audio_de"
        o = self._run(iq_block, [au, "demod"] if return_demod else [au])
        return (o[au], o["demod"]) if return_demod else o[au]

    def pcm(self) -> np.ndarray:
        """The latest block as interleaved int16 PCM (2 A values; needs deemphasis=tau)."""
        return self.rx.pcm()[0]

    @property
    def phase(self) -> float:
        """The carried demod phase (model/fmSupportLib.py:40-44)."""
        return float(self.rx.state()[0][0])


class StereoBlockProcessor(MonoBlockProcessor):
    """Mono + stereo (model/fmMonoBlock.py:113-173, intended combiner L=(a+s)/2, R=(a-s)/2)."""

    _mode = dict(mono=True, stereo=True)

    def __init__(self, block_complex: int, rf_coeff=None, audio_coeff=None, stereo_taps: int = 151, **kw):
        super().__init__(block_complex, rf_coeff, audio_coeff, stereo_taps=stereo_taps, **kw)

    def process(self, iq_block, return_intermediates: bool = False):
        names = ["audio", "stereo", "left", "right"]
        if self.rx.deemphasis is not None:
            names += ["audio_de", "left_de", "right_de"]
        if return_intermediates:
            names += ["demod", "bpf_recovery", "nco", "bpf_extraction"]
        return self._run(iq_block, names)


class RdsBlockProcessor(MonoBlockProcessor):
    """RDS signal path of model/fmRDSblock.py:156-204, from the demod stream to the RRC
    output (I and Q).  The bit-level link layer after :204 is RdsLinkLayer."""

    _mode = dict(mono=False, rds=True)

    def __init__(self, block_complex: int = 153600, rf_coeff=None, taps: int = 151, iq_dtype=np.uint8, **kw):
        super().__init__(block_complex, rf_coeff, None, iq_dtype=iq_dtype, rds_taps=taps, **kw)
        self.R = self.rx.R

    def process(self, iq_block, return_intermediates: bool = False):
        names = ["rrc_i", "rrc_q"]
        if return_intermediates:
            names += ["demod", "extract", "pre_pll", "nco_i", "nco_q", "lpf_i", "lpf_q", "resample_i",
                      "resample_q"]
        return self._run(iq_block, names)


class RdsLinkLayer(_Handle):
    """RDS link layer of model/fmRDSblock.py:207-346 on the host (libsdr C++, no GPU):
    clock and data recovery, Manchester and differential decoding, syndrome frame sync.

    process(rrc_i) takes one block of the in-phase RRC output (RdsBlockProcessor's
    'rrc_i') and returns dict(events=[(type, position, accepted)], symbols, bits, diff):
    type 0..3 = syndrome A..D, accepted = the reference's "Syndrome X at position N"
    prints (1) or its "False positive" prints (0); the state carries across calls."""

    TYPES = "ABCD"
    RESYNC = 4
    _prefix = "sdr_rds_link"

    def __init__(self, resync_after: int = 0):
        """resync_after > 0: the C++ frame_thread's rule (src/fm_radio.cpp:697-704; it uses
        10) -- after that many false positives in a row the frame position is forgotten and a
        (RESYNC, position, 0) event is reported.  0: the Python model's behaviour."""
        import ctypes
        self._c = ctypes
        self.lib = _lib.load_library()
        h = ctypes.c_void_p()
        check(self.lib.sdr_rds_link_create(ctypes.byref(h)), "sdr_rds_link_create")
        self.handle = h
        if resync_after:
            check(self.lib.sdr_rds_link_set_resync(h, int(resync_after)), "sdr_rds_link_set_resync")

    def process(self, rrc_i):
        c = self._c
        x = np.ascontiguousarray(rrc_i, dtype=np.float64)
        n = len(x)
        ns_max = n // 24 + 2
        nb_max = ns_max // 2 + 2
        nd_max = nb_max + 64
        ev = np.empty(3 * (nd_max + 1), dtype=np.int64)
        sym = np.empty(ns_max)
        bits = np.empty(nb_max, dtype=np.uint8)
        diff = np.empty(nd_max, dtype=np.uint8)
        ne, ns, nb, nd = c.c_int64(), c.c_int64(), c.c_int64(), c.c_int64()
        vp = lambda a: a.ctypes.data_as(c.c_void_p)  # noqa: E731
        check(self.lib.sdr_rds_link_block(self.handle, f64p(x), n, vp(ev), nd_max + 1, c.byref(ne), vp(sym),
                                          ns_max, c.byref(ns), vp(bits), nb_max, c.byref(nb), vp(diff), nd_max,
                                          c.byref(nd)), "sdr_rds_link_block")
        events = [tuple(int(v) for v in ev[3 * k:3 * k + 3]) for k in range(ne.value)]
        return dict(events=events, symbols=sym[:ns.value].copy(), bits=bits[:nb.value].copy(),
                    diff=diff[:nd.value].copy())


class _RdsBank(_Handle):
    """An RDS stage for `S` streams at once on the GPU, every stream's state in device memory: the
    context, the create with the set-up that follows it, the stream-count rule, the receiver's
    rows and the int64 state matrix."""

    @contextlib.contextmanager
    def _create(self, nstreams, ctx, *args):
        """<prefix>_create(context, S, *args, &handle) on `ctx` (None: the default context); a
        failure of the set-up in the `with` body closes the object again."""
        self.S = int(nstreams)
        self.ctx = ctx if ctx is not None else _lib.get_context()
        self.lib = self.ctx.lib
        h = ctypes.c_void_p()
        name = f"{self._prefix}_create"
        check(getattr(self.lib, name)(self.ctx.handle, self.S, *args, ctypes.byref(h)), name)
        self.handle = h
        try:
            yield
        except Exception:
            self.close()
            raise

    def _check_streams(self, other, noun, me="bank"):
        if other.S != self.S:
            raise ValueError(f"the {noun} has {other.S} streams, the {me} {self.S}")

    def _receiver_rows(self, receiver, *names):
        """(pointer per name, n, stride) of the receiver's latest rows of those names."""
        self._check_streams(receiver, "receiver")
        rows = [receiver.output_ptr(name) for name in names]
        if any(r[1:] != rows[0][1:] for r in rows):
            raise ValueError(f"the receiver's {' and '.join(names)} rows differ in shape")
        return (*(r[0] for r in rows), rows[0][2], rows[0][1])

    def _state_rows(self, ncols):
        st = np.zeros((self.S, ncols), dtype=np.int64)
        self._do("state", st.ctypes.data)
        return [tuple(int(v) for v in row) for row in st]

    def reset(self):
        """Every stream back to its start (block 0, SEARCH at position 0, sample 0); the counters
        to 0."""
        self._do("reset")


class RdsLinkBank(_RdsBank):
    """RdsLinkLayer for `nstreams` streams at once, on the GPU (sdr_rds_links, csrc/rds.hip): the
    in-phase RRC rows are read where the receiver left them, every stream's link state stays in
    device memory, and what comes back is the events -- per stream a list of
    (type, position, accepted, word), the first three as RdsLinkLayer reports them and `word` the
    block's 16 information bits (0 for a RESYNC).  Bits, scanned bits, events and state equal
    RdsLinkLayer's on the same float32 samples, call by call.

    max_n: the longest row a call may bring (a call takes MIN_N <= n <= max_n samples per row).
    max_events: events kept per stream and call (default: two per window -- no call can give more
    -- up to 4096); beyond it the excess is dropped, `counts` still has the true number and
    `status` OVERFLOW.
    resync_after: as RdsLinkLayer's."""

    TYPES = "ABCD"
    RESYNC = 4
    MIN_N = _lib.SDR_RDS_LINKS_MIN_N
    FAULT, OVERFLOW = _lib.SDR_RDS_LINKS_FAULT, _lib.SDR_RDS_LINKS_OVERFLOW
    _prefix = "sdr_rds_links"

    def __init__(self, nstreams: int, max_n: int, *, max_events=None, resync_after: int = 0, ctx=None):
        self.max_n = int(max_n)
        # a call scans at most (max_n / 24) / 2 + 2 windows, and a window gives at most two events
        self.max_events = int(max_events) if max_events is not None else min(2 * (self.max_n // 48 + 4), 4096)
        with self._create(nstreams, ctx, self.max_n, self.max_events):
            self.counts = np.zeros(self.S, dtype=np.int64)
            if resync_after:
                self.set_resync(resync_after)

    def set_resync(self, after_bad_syncs: int):
        self._do("set_resync", int(after_bad_syncs))

    def process_dev(self, ptr: int, n: int, stride: int):
        """One call for every stream: row s is the n floats at device pointer ptr + 4 s stride.
        Async on the context stream."""
        self._do("process_dev", ptr, int(n), int(stride))

    def process_rx(self, receiver: "Receiver"):
        """The receiver's latest "rrc_i" rows (looked up at every call: a pipelined receiver
        alternates its row sets; call it before the receiver's next process_dev, which keeps the
        rows until this call has read them)."""
        self.process_dev(*self._receiver_rows(receiver, "rrc_i"))

    def events(self):
        """(events, status) of the last call, after waiting for it: events[s] the stream's list of
        (type, position, accepted, word), status[s] 0 or FAULT / OVERFLOW bits; `counts` is set
        to the true event counts."""
        ev = np.zeros((self.S, self.max_events, 4), dtype=np.int64)
        ne = np.zeros(self.S, dtype=np.int64)
        status = np.zeros(self.S, dtype=np.int32)
        self._do("events", ev.ctypes.data, ne.ctypes.data, status.ctypes.data)
        self.counts = ne
        return [[tuple(e) for e in ev[s, :min(int(ne[s]), self.max_events)].tolist()] for s in range(self.S)], status

    def bits(self, stream: int):
        """(bits, diff) of the last call for one stream: the Manchester bits and the scanned row
        (carried bits first), uint8 -- RdsLinkLayer's 'bits' and 'diff'."""
        nb_max = self.max_n // 48 + 2
        bits, diff = np.empty(nb_max, dtype=np.uint8), np.empty(nb_max + 32, dtype=np.uint8)
        nb, nd = ctypes.c_int64(), ctypes.c_int64()
        self._do("bits", int(stream), bits.ctypes.data, len(bits), ctypes.byref(nb), diff.ctypes.data, len(diff), ctypes.byref(nd))
        return bits[:nb.value].copy(), diff[:nd.value].copy()

    def block_sync(self, **kw) -> "RdsSyncBank":
        """A device-side block synchroniser sized to this bank (RdsSyncBank: one stream per link
        stream, max_bits what one link call can add); feed it with sync.process_links(bank)
        after each link call."""
        kw.setdefault("ctx", self.ctx)
        return RdsSyncBank(self.S, -(-self.max_n // 24) // 2, **kw)


class RdsSyncBank(_RdsBank):
    """RDS block synchronisation for `nstreams` streams at once, on the GPU (sdr_rds_sync,
    csrc/rds_sync.hip): acquisition, flywheel, burst correction and offset C' over every stream's
    differential bits, all state in device memory.  rdssync.RdsBlockSync is the specification:
    records, state and counters equal it after every call, whatever the split.

    max_bits: the most bits a call may bring per stream.  max_burst, lose_after: as
    RdsBlockSync's.  blocks() returns the last call's records, per stream a list of
    (type, position, status, word) -- what RdsProgramme.feed takes."""

    TYPES = ("A", "B", "C", "D", "C'")
    _prefix = "sdr_rds_sync"

    def __init__(self, nstreams: int, max_bits: int, max_burst: int = 2, lose_after: int = 12, ctx=None):
        self.max_bits = int(max_bits)
        self.max_records = self.max_bits // 26 + 3
        with self._create(nstreams, ctx, self.max_bits):
            self.set_params(max_burst, lose_after)

    def set_params(self, max_burst: int, lose_after: int):
        self._do("set_params", int(max_burst), int(lose_after))
        self.max_burst, self.lose_after = int(max_burst), int(lose_after)

    def process_dev(self, ptr: int, n: int, stride: int, counts_ptr: int = 0):
        """One call for every stream: row s is the n bytes at device pointer ptr + s stride, bit 0
        of each byte a bit.  counts_ptr: 0 (every stream takes n bits) or a device array of
        nstreams int32 counts 0 .. n.  Async on the context stream."""
        self._do("process_dev", ptr, int(n), int(stride), counts_ptr or None)

    def process_links(self, bank: "RdsLinkBank"):
        """Every stream takes the scanned bits the link bank's last call added (none where it
        faulted).  Async on the context stream; call it once after each link call."""
        self._do("process_links", bank.handle)

    def blocks(self):
        """The last call's records, after waiting for it: per stream a list of 4-tuples."""
        rec = np.zeros((self.S, self.max_records, 4), dtype=np.int64)
        nr = np.zeros(self.S, dtype=np.int64)
        self._do("blocks", rec.ctypes.data, nr.ctypes.data)
        return [[tuple(r) for r in rec[s, :min(int(nr[s]), self.max_records)].tolist()] for s in range(self.S)]

    def state(self):
        """Per stream (synced, next position, blocks of status 0, 1, 2, acquisitions, losses) --
        RdsBlockSync.state() -- after waiting for the last call."""
        synced = np.zeros(self.S, dtype=np.int32)
        pos = np.zeros(self.S, dtype=np.int64)
        cnt = np.zeros((self.S, 5), dtype=np.int64)
        self._do("state", synced.ctypes.data, pos.ctypes.data, cnt.ctypes.data)
        return [(int(synced[s]), int(pos[s]), *(int(v) for v in cnt[s])) for s in range(self.S)]


class RdsClockBank(_RdsBank):
    """RDS symbol clock recovery for `nstreams` streams at once, on the GPU (sdr_rds_clock,
    csrc/rds_clock.hip): the in-phase RRC rows are read where the receiver left them, and every
    stream's differential bits (byte per bit) and an int32 count per stream stay in device memory
    for RdsSyncBank.process_dev -- feed(sync).  Where RdsLinkBank keeps the sampling offset of the
    first 24 samples for ever, this follows the symbol clock: a receiver whose crystal is off keeps
    its bits.  rdsclock.RdsSymbolClock is the specification: bits, counts and state equal it
    after every call, whatever the split.

    max_n: the longest row a call may bring (0 <= n <= max_n).  window, hysteresis: as
    RdsSymbolClock's.  max_bits: the most bits a call can give per stream."""

    _prefix = "sdr_rds_clock"

    def __init__(self, nstreams: int, max_n: int, window: int = 4, hysteresis: int = 8, ctx=None):
        self.max_n = int(max_n)
        with self._create(nstreams, ctx, self.max_n):
            self.set_params(window, hysteresis)
            dev, cnt = ctypes.c_void_p(), ctypes.c_void_p()
            stride, mb = ctypes.c_int64(), ctypes.c_int64()
            self._do("bits", ctypes.byref(dev), ctypes.byref(stride), ctypes.byref(cnt), ctypes.byref(mb))
        self.bits_ptr, self.bits_stride, self.counts_ptr, self.max_bits = dev.value, stride.value, cnt.value, mb.value

    def set_params(self, window: int, hysteresis: int):
        """For the calls that follow (the model takes them at construction: set them before the
        first call to equal it)."""
        self._do("set_params", int(window), int(hysteresis))
        self.window, self.hysteresis = int(window), int(hysteresis)

    def process_dev(self, ptr: int, n: int, stride: int):
        """One call for every stream: row s is the n floats at device pointer ptr + 4 s stride,
        0 <= n <= max_n.  Async on the context stream."""
        self._do("process_dev", ptr, int(n), int(stride))

    def process_rx(self, receiver: "Receiver"):
        """The receiver's latest "rrc_i" rows (looked up at every call: a pipelined receiver
        alternates its row sets; call it before the receiver's next process_dev, which keeps the
        rows until this call has read them)."""
        self.process_dev(*self._receiver_rows(receiver, "rrc_i"))

    def bits(self):
        """The last call's differential bits, after waiting for it: per stream a uint8 array."""
        b = np.zeros((self.S, self.max_bits), dtype=np.uint8)
        cnt = np.zeros(self.S, dtype=np.int32)
        self._do("fetch", b.ctypes.data, cnt.ctypes.data)
        return [b[s, :int(cnt[s])].copy() for s in range(self.S)]

    def state(self):
        """Per stream (consumed samples, segments, phi, pi, symbols, bits, steps forward, steps
        back, wraps, pairing changes) -- RdsSymbolClock.state() -- after waiting for the last call."""
        return self._state_rows(_lib.SDR_RDS_CLOCK_NSTATE)

    def block_sync(self, **kw) -> "RdsSyncBank":
        """A device-side block synchroniser sized to this bank (RdsSyncBank: one stream per clock
        stream, max_bits what one call of max_n can add); feed it with bank.feed(sync) after each
        call."""
        kw.setdefault("ctx", self.ctx)
        return RdsSyncBank(self.S, self.max_bits, **kw)

    def feed(self, sync: "RdsSyncBank"):
        """The last call's bits into the block synchroniser, device to device: every stream takes
        its own count.  Async on the context stream; call it once after each call."""
        self._check_streams(sync, "sync")
        sync.process_dev(self.bits_ptr, self.max_bits, self.bits_stride, self.counts_ptr)


class RdsCarrierBank(_RdsBank):
    """RDS carrier phase recovery for `nstreams` streams at once, on the GPU (sdr_rds_carrier,
    csrc/rds_carrier.hip): the "rrc_i" and "rrc_q" rows are read where the receiver left them, and
    one row per stream -- the samples projected onto the axis the data lie on -- stays in device
    memory for RdsClockBank.process_dev or RdsLinkBank.process_dev: feed(bank).  n samples in give
    n samples out.  rdscarrier.RdsCarrierPhase is the specification: rows, state and moments equal
    it after every call, whatever the split.

    max_n: the longest row a call may bring (0 <= n <= max_n).  window: as RdsCarrierPhase's.
    rows_ptr, rows_stride: the device rows, rows_stride floats apart."""

    _prefix = "sdr_rds_carrier"

    def __init__(self, nstreams: int, max_n: int, window: int = 8, ctx=None):
        self.max_n = int(max_n)
        self.n = 0                                                # the last call's
        with self._create(nstreams, ctx, self.max_n):
            self.set_params(window)
            dev, stride = ctypes.c_void_p(), ctypes.c_int64()
            self._do("rows", ctypes.byref(dev), ctypes.byref(stride))
        self.rows_ptr, self.rows_stride = dev.value, stride.value

    def set_params(self, window: int):
        """For the calls that follow (the model takes it at construction: set it before the first
        call to equal it)."""
        self._do("set_params", int(window))
        self.window = int(window)

    def process_dev(self, i_ptr: int, q_ptr: int, n: int, stride: int):
        """One call for every stream: row s of i and of q is the n floats at device pointer
        i_ptr + 4 s stride and q_ptr + 4 s stride, 0 <= n <= max_n.  Async on the context stream."""
        self._do("process_dev", i_ptr, q_ptr, int(n), int(stride))
        self.n = int(n)

    def process_rx(self, receiver: "Receiver"):
        """The receiver's latest "rrc_i" and "rrc_q" rows (looked up at every call: a pipelined
        receiver alternates its row sets; call it before the receiver's next process_dev, which
        keeps the rows until this call has read them)."""
        self.process_dev(*self._receiver_rows(receiver, "rrc_i", "rrc_q"))

    def rows(self) -> np.ndarray:
        """The last call's rows, after waiting for it: (nstreams, n) float32."""
        out = np.empty((self.S, self.n), dtype=np.float32)
        self._do("fetch", out.ctypes.data, self.n)
        return out

    def state(self):
        """Per stream (consumed samples, complete segments, kappa, steps forward, steps back, holds,
        wraps) -- RdsCarrierPhase.state() -- after waiting for the last call."""
        return self._state_rows(_lib.SDR_RDS_CARRIER_NSTATE)

    def moments(self):
        """Per stream (A, B, C) of the window behind the last complete segment's direction --
        RdsCarrierPhase.moments() -- after waiting for the last call."""
        m = np.zeros((self.S, 3), dtype=np.float64)
        self._do("moments", m.ctypes.data)
        return [tuple(float(v) for v in row) for row in m]

    def reset(self):
        """Every stream back to sample 0; the counters to 0."""
        super().reset()
        self.n = 0

    def feed(self, bank):
        """The last call's rows into an RdsClockBank or an RdsLinkBank, device to device.  Async on
        the context stream; call it once after each call."""
        self._check_streams(bank, "bank", "carrier stage")
        bank.process_dev(self.rows_ptr, self.n, self.rows_stride)

    def clock(self, **kw) -> "RdsClockBank":
        """A device-side symbol clock sized to this bank; feed it with bank.feed(clock) after each
        call."""
        kw.setdefault("ctx", self.ctx)
        return RdsClockBank(self.S, self.max_n, **kw)


def rds_groups(events):
    """One stream's events -> the groups in them: an accepted A at position p with accepted B, C,
    D at p + 26, p + 52, p + 78 gives (pi, b, c, d), the four blocks' information words.  Takes
    the 4-tuples of RdsLinkBank.events()."""
    ok = {(int(e[1]), int(e[0])): int(e[3]) for e in events if len(e) >= 4 and e[2] and 0 <= e[0] < 4}
    groups = []
    for (p, t) in sorted(ok):
        if t == 0 and all((p + 26 * k, k) in ok for k in (1, 2, 3)):
            groups.append(tuple(ok[(p + 26 * k, k)] for k in range(4)))
    return groups


class _IngestParamsC(ctypes.Structure):                          # include/sdr.h sdr_ingest_params
    _fields_ = [("bits", ctypes.c_int), ("swap", ctypes.c_int), ("meter", ctypes.c_int)]


class _IngestMeterC(ctypes.Structure):                           # include/sdr.h sdr_ingest_meter
    _fields_ = ([(k, ctypes.c_int64) for k in ("n", "clipped", "nonfinite", "peak_code")] + [("sumsq_code", ctypes.c_uint64)] +
                [(k, ctypes.c_double) for k in ("peak", "sumsq")] + [(k, ctypes.c_int64) for k in ("calls", "total_n", "total_clipped")])


class CaptureIngest(_LazyHandle):
    """The raw bytes of a capture block to the float32 capture on the GPU, with a level meter
    (sdr_ingest, csrc/ingest.hip): the stage in front of IqCorrector.  `fmt` is 'cu8', 'cs8', 'cs16'
    or 'cf32' (or numpy's uint8, int8, int16, float32; capture_format maps file and SigMF names);
    `bits` is the width of the ADC's code in a cs16 word (12 for a 12-bit ADC); swap exchanges I and
    Q.  process_dev reads the bytes in device memory -- a quarter (cs8) or half (cs16) of what the
    float32 block would have cost to upload -- and writes interleaved float32, out = code 2^-(bits - 1),
    the buffer every stage behind it reads.  With meter=True a second, one-wave launch leaves the
    call's meter in device memory: the samples on a rail, the peak and the sum of squares of the
    ADC's codes, exact, and the totals over calls; meter() fetches it (IngestMeter: power_dbfs,
    peak_dbfs, clip_share).  With meter=False the stage is the conversion alone and the meter stays
    zero.  Nothing returns to the host unless meter() is asked.

    The rule is rtsdr.ingest_model's (capture.py), bit for bit.  For cf32 the block passes through
    unchanged (swap aside) and out_ptr == raw_ptr is allowed.  The arguments are checked before a
    context exists; the device object is made at the first call that needs it."""

    CHUNK = _lib.SDR_INGEST_CHUNK                                # samples of a workgroup's chunk (at least)
    MAX_N = capture.MAX_N
    _prefix = "sdr_ingest"
    _DTYPES = {"cf32": _lib.SDR_IQ_F32, "cu8": _lib.SDR_IQ_U8, "cs8": _lib.SDR_IQ_S8, "cs16": _lib.SDR_IQ_S16}

    def __init__(self, fmt, bits=None, swap: bool = False, meter: bool = True, ctx=None):
        self.fmt, self.bits = capture.check_format(fmt, bits)
        self.swap, self.metered = bool(swap), bool(meter)
        self.es = 2 * capture.FORMATS[self.fmt][0].itemsize      # bytes of a complex sample
        self._ctx = ctx

    def _create_args(self):
        return self._DTYPES[self.fmt], ctypes.byref(_IngestParamsC(self.bits, int(self.swap), int(self.metered)))

    def process_dev(self, raw_ptr: int, n: int, out_ptr: int):
        """n complex samples of the format at device pointer raw_ptr -> n complex float32 at out_ptr;
        async on the context stream."""
        self._do("process_dev", *_check_capture_call("raw", raw_ptr, self.es, n, out_ptr, self.fmt == "cf32", "a cf32 ingest"))

    def run(self, raw) -> np.ndarray:
        """A capture block from the host (values of the format's type, raw bytes, or complex64 for
        cf32) -> interleaved float32 (2 n values); synchronous (sdr_ingest_run)."""
        raw = capture.as_raw(raw, self.fmt)
        n = raw.size // 2
        out = np.empty(2 * n, dtype=np.float32)
        self._do("run", raw.ctypes.data, n, out.ctypes.data)
        return out

    def meter(self) -> "capture.IngestMeter":
        """The meter of the last call and the totals since the last reset (sdr_ingest_meter_get;
        synchronises)."""
        m = _IngestMeterC()
        self._do("meter_get", ctypes.byref(m))
        return capture.IngestMeter(*(getattr(m, k) for k in capture.IngestMeter._fields))

    @property
    def meter_ptr(self) -> int:
        """The device copy of the meter, a struct sdr_ingest_meter (sdr_ingest_meter_dev)."""
        return self._ptr_out("meter_dev")

    def reset(self):
        """Zero the meter and its totals (async)."""
        self._do("reset")


class _IqcParamsC(ctypes.Structure):                             # include/sdr.h sdr_iqc_params
    _fields_ = [("rate", ctypes.c_double), ("dc", ctypes.c_int), ("balance", ctypes.c_int)]


class IqCorrector(_Timed, _LazyHandle):
    """IQ imbalance and DC offset correction of a capture block on the GPU (sdr_iqc, csrc/iqc.hip):
    the stage in front of Spectrum, Channelizer and FilterBank.  A direct-conversion front end's Q
    branch has a slightly different gain and is not quite 90 degrees from I, so every station at +f
    leaves an image at -f, in another channel of the bank; and the ADC's zero is not zero, a carrier
    in the centre bin.  process_dev reads a block in device memory (interleaved float32, or uint8
    as (x - 128) / 128), estimates both from the block's five second moments, smooths the estimate
    over calls by `rate`, and writes the corrected block as interleaved float32 -- the buffer the
    stages behind it read.  Three launches, nothing returns to the host unless state() is asked.

    The rule is rtsdr.IqBalance's (iqbalance.py), step for step; it is blind (no pilot, no
    calibration tone) and frequency-independent: one 2 x 2 matrix for the whole band.  dc=False /
    balance=False leave that half of the correction out.  estimate=False applies the coefficients
    in force without looking at the block; set() installs coefficients of a front end calibrated
    once.  For float32, out_ptr == iq_ptr (in place) is allowed.  The arguments are checked before
    a context exists; the device object is made at the first call that needs it."""

    NSTATE = _lib.SDR_IQC_NSTATE
    CHUNK = _lib.SDR_IQC_CHUNK                                   # samples of a workgroup's chunk (at least)
    MAX_N = 2 ** 31 - 1
    _prefix = "sdr_iqc"
    _STAGES = ("moments", "update", "apply")                     # stage_ms: the last call made with an estimate

    def __init__(self, iq_dtype=np.float32, rate: float = iqbalance.DEFAULT_RATE, dc: bool = True, balance: bool = True, ctx=None):
        self.u8 = _is_u8(iq_dtype)
        self.rate, self.dc, self.balance = iqbalance.check_rate(rate), bool(dc), bool(balance)
        self._ctx = ctx

    def _create_args(self):
        return SDR_IQ_U8 if self.u8 else SDR_IQ_F32, ctypes.byref(_IqcParamsC(self.rate, int(self.dc), int(self.balance)))

    def process_dev(self, iq_ptr: int, n: int, out_ptr: int, estimate: bool = True):
        """n complex samples at device pointer iq_ptr -> n corrected complex float32 at out_ptr;
        async on the context stream."""
        args = _check_capture_call("iq", iq_ptr, 2 if self.u8 else 8, n, out_ptr, not self.u8, "a float32 corrector")
        self._do("process_dev", *args, int(bool(estimate)))

    def run(self, iq, estimate: bool = True) -> np.ndarray:
        """n complex samples from the host (interleaved f32 / u8, or complex for a float32 object)
        -> the corrected block, interleaved float32 (2 n values); synchronous (sdr_iqc_run)."""
        iq = _interleaved_iq(iq, self.u8, "corrector")
        n = iq.size // 2
        if not 1 <= n <= self.MAX_N:
            raise ValueError(f"n={n} outside [1, 2^31 - 1]")
        out = np.empty(2 * n, dtype=np.float32)
        self._do("run", iq.ctypes.data, n, out.ctypes.data, int(bool(estimate)))
        return out

    def raw_state(self) -> np.ndarray:
        """The 12 float64 values mI mQ pII pQQ pIQ dI dQ c1 c2 updates skipped holds (sdr_iqc_state;
        synchronises)."""
        out = np.empty(self.NSTATE)
        self._do("state", f64p(out))
        return out

    def state(self) -> "iqbalance.IqState":
        """The state as IqBalance.state() gives it: the 12 values, and impropriety / image_db of the
        smoothed moments computed on the host."""
        return iqbalance.make_state(self.raw_state())

    def set(self, dI: float, dQ: float, c1: float, c2: float):
        """Install coefficients (async); the next estimate replaces them."""
        c = np.array(iqbalance.check_coeffs((dI, dQ, c1, c2)))
        self._do("set", f64p(c))

    def reset(self):
        """Back to the state after creation (async)."""
        self._do("reset")

    @property
    def coeffs_ptr(self) -> int:
        """The device array of four float64 dI dQ c1 c2 (sdr_iqc_coeffs_dev)."""
        return self._ptr_out("coeffs_dev")


class Channelizer(_DecimBlock):
    """One wideband IQ capture to `len(freqs_hz)` receiver streams on the GPU (sdr_ddc,
    csrc/ddc.hip): per channel "mix down by freqs_hz[c], lfilter(taps, 1, .), [::decim]", all
    channels in one matrix-core launch.  The reference has no channelizer; this is the stage in
    front of a Receiver when one front end carries several stations.

    freqs_hz: the channel centres relative to the capture's centre, |f| <= fs / 2.  The
    oscillators are 32-bit integer phase accumulators on the absolute sample index (exact at
    any stream position and across any split into calls): `freqs_hz` then reads the quantised
    frequencies, a multiple of fs / 2^32 each.  taps: an array of real FIR taps, a tap count,
    or None (design.channel_coeffs(decim, taps): firwin at the output Nyquist).  The filter
    history and the stream position are carried from call to call; every call takes a
    multiple of `decim` samples.

    process(iq) takes interleaved IQ (2 n values, f32 or u8) or a complex array and returns
    the (nch, n / decim) complex64 rows; process_dev works on device memory in place: row c
    starts 2 c out_stride floats into `out_ptr` -- the layout Receiver.process_dev reads with
    iq_stride = out_stride."""

    MAX_CH, MAX_TAPS, MAX_DECIM = 64, 256, 64      # include/sdr.h SDR_DDC_MAX_*
    WINDOW = 64                                    # outputs per wave window (SDR_DDC_WINDOW)
    _prefix, _noun = "sdr_ddc", "channelizer"

    def __init__(self, freqs_hz, fs: float, decim: int, taps=None, iq_dtype=np.float32, ctx=None):
        fs, decim = float(fs), int(decim)
        if not (np.isfinite(fs) and fs > 0):
            raise ValueError("fs must be positive")
        if not 1 <= decim <= self.MAX_DECIM:
            raise ValueError(f"decim={decim} outside [1, {self.MAX_DECIM}]")
        f = np.atleast_1d(np.asarray(freqs_hz, dtype=np.float64))
        if f.ndim != 1 or not 1 <= len(f) <= self.MAX_CH:
            raise ValueError(f"{f.shape} channel frequencies: 1..{self.MAX_CH} channels")
        if not np.all(np.isfinite(f)) or np.any(np.abs(f / fs) > 0.5):
            raise ValueError("channel frequencies must be finite and within [-fs/2, fs/2]")
        b = _real_taps(taps, self.MAX_TAPS, lambda t: design.channel_coeffs(decim, t), count_checked=False)
        self.u8 = _is_u8(iq_dtype)
        self.fs, self.decim, self.taps, self.nch = fs, decim, b, len(f)
        self.inc = [design.ddc_phase_inc(v / fs) for v in f]
        self.ctx = ctx if ctx is not None else _lib.get_context()
        self.lib = self.ctx.lib
        nu = np.ascontiguousarray(f / fs)
        h = ctypes.c_void_p()
        check(self.lib.sdr_ddc_create(self.ctx.handle, self.nch, f64p(nu), f64p(b), len(b), decim,
                                      SDR_IQ_U8 if self.u8 else SDR_IQ_F32, ctypes.byref(h)), "sdr_ddc_create")
        self.handle = h

    @property
    def freqs_hz(self) -> np.ndarray:
        """The frequencies in use (sdr_ddc_freq): signed(inc) / 2^32 x fs."""
        nu = np.empty(self.nch)
        check(self.lib.sdr_ddc_freq(self.handle, f64p(nu)), "sdr_ddc_freq")
        return nu * self.fs


class FilterBank(_DecimBlock):
    """A polyphase filter bank on the GPU (sdr_pfb, csrc/pfb.hip): one wideband IQ capture to
    the selected bins of a uniform grid of `nbins` across the capture, bin k centred on
    k / nbins x fs (bins >= nbins / 2 are the negative frequencies), each at fs / decim.  Per
    channel it is Channelizer's "mix down, lfilter(taps, 1, .), [::decim]" with the oscillator
    on the grid -- its phase ((bin k) mod nbins) / nbins turns at absolute sample index k, exact
    integer arithmetic -- but the filter is folded once for all channels and only an
    nbins-point DFT is per channel, so the channel count does not multiply the filter's work:
    the front end for a whole band of uniformly spaced stations.

    bins: the selected bins, in any order, repeats allowed, unsigned in [0, nbins) or signed in
    [-nbins/2, nbins/2) (reduced mod nbins); None selects all of them in order.  taps: an array
    of real prototype taps, a tap count, or None (design.pfb_coeffs(nbins): firwin at half the
    bin spacing, 8 taps per bin).  decim is free: it need not divide nbins.  The filter history
    and the stream position are carried from call to call; every call takes a multiple of
    `decim` samples.

    process / process_dev / reset / position / close are Channelizer's, the rows laid out the
    same way: row c starts 2 c out_stride floats into `out_ptr`, what Receiver.process_dev reads
    with iq_stride = out_stride."""

    MAX_BINS, MAX_CH, MAX_TAPS, MAX_DECIM = 256, 256, 4096, 64      # include/sdr.h SDR_PFB_MAX_*
    WINDOW = 64                                                     # output times per window (SDR_PFB_WINDOW)
    _prefix, _noun = "sdr_pfb", "filter bank"

    def __init__(self, nbins: int, fs: float, decim: int, bins=None, taps=None, iq_dtype=np.float32, ctx=None):
        nbins, fs, decim = int(nbins), float(fs), int(decim)
        if not (np.isfinite(fs) and fs > 0):
            raise ValueError("fs must be positive")
        if not 1 <= nbins <= self.MAX_BINS:
            raise ValueError(f"nbins={nbins} outside [1, {self.MAX_BINS}]")
        if not 1 <= decim <= self.MAX_DECIM:
            raise ValueError(f"decim={decim} outside [1, {self.MAX_DECIM}]")
        k = np.arange(nbins) if bins is None else np.atleast_1d(np.asarray(bins))
        if k.ndim != 1 or not 1 <= len(k) <= self.MAX_CH:
            raise ValueError(f"{k.shape} bins: 1..{self.MAX_CH} channels")
        if not np.all(np.isfinite(k)) or np.any(k != np.rint(k)):
            raise ValueError("bins must be integers")
        k = k.astype(np.int64)
        if np.any(2 * k < -nbins) or np.any(k >= nbins):
            raise ValueError(f"bins must lie in [-nbins/2, nbins) with nbins={nbins}")
        def designed(count):                        # a tap count: the same prototype at that length
            if count is None:
                return design.pfb_coeffs(nbins)
            return design.signal.firwin(int(count), 1.0 / nbins) if nbins > 1 else np.eye(1, int(count))[0]
        b = _real_taps(taps, self.MAX_TAPS, designed)
        self.u8 = _is_u8(iq_dtype)
        self.nbins, self.fs, self.decim, self.taps = nbins, fs, decim, b
        self.bins = np.ascontiguousarray(k % nbins, dtype=np.int32)
        self.nch = len(self.bins)
        self.ctx = ctx if ctx is not None else _lib.get_context()
        self.lib = self.ctx.lib
        h = ctypes.c_void_p()
        check(self.lib.sdr_pfb_create(self.ctx.handle, nbins, self.nch, self.bins.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                      f64p(b), len(b), decim, SDR_IQ_U8 if self.u8 else SDR_IQ_F32, ctypes.byref(h)),
              "sdr_pfb_create")
        self.handle = h

    @property
    def freqs_hz(self) -> np.ndarray:
        """The channel centres: signed(bin) / nbins x fs (bins >= nbins / 2 are negative)."""
        k = self.bins.astype(np.int64)
        return np.where(2 * k >= self.nbins, k - self.nbins, k) / self.nbins * self.fs


class RowResampler(_Stream):
    """A rational up / down resampler for `nrows` rows of device memory (sdr_rsmp,
    csrc/rsmp.hip), complex or real f32: the stage between a channelizer or filter bank whose
    fs / decim is not the receiver's 2.4 MS/s and the Receiver (2.5 MS/s rows x 24/25), or N
    audio streams 48 kHz -> 44.1 kHz (147/160).  Per row and component
    up x lfilter(taps, 1, zero-stuff(x, up))[::down] (= up x scipy.signal.upfirdn(taps, x, up,
    down) cut to length), as a polyphase f32 FMA chain per output.

    taps: an array of real taps designed at `up` times the input rate, a tap count, or None
    (design.resample_coeffs(up, down): scipy.signal.resample_poly's default filter; with it and
    down >= up, output m + 10 is resample_poly(x, up, down)[m]).  At most MAX_TAPS taps and
    MAX_PHASE_TAPS per phase (ceil(taps / up)).  Every call takes n samples per row with
    n up % down == 0 and gives n up / down; the last ceil(taps / up) - 1 samples of every row
    and the position are carried from call to call, and any split of a stream into calls gives
    the same bits as one call.

    process(x) takes a host (nrows, n) complex64 (float32 for a real object) array and returns
    (nrows, n up / down); process_dev works on device memory in place: row r starts r stride
    samples into its buffer -- a complex object's output rows are what Receiver.process_dev
    reads with iq_stride = out_stride."""

    MAX_FACTOR, MAX_TAPS, MAX_PHASE_TAPS, MAX_ROWS = 1024, 4096, 256, 65535      # include/sdr.h SDR_RSMP_MAX_*
    TILE = 2048                                                                  # outputs a workgroup produces as a unit (SDR_RSMP_TILE)
    _prefix = "sdr_rsmp"

    def __init__(self, nrows: int, up: int, down: int, taps=None, complex: bool = True, ctx=None):
        nrows, up, down = int(nrows), int(up), int(down)
        if not 1 <= nrows <= self.MAX_ROWS:
            raise ValueError(f"nrows={nrows} outside [1, {self.MAX_ROWS}]")
        if not 1 <= up <= self.MAX_FACTOR:
            raise ValueError(f"up={up} outside [1, {self.MAX_FACTOR}]")
        if not 1 <= down <= self.MAX_FACTOR:
            raise ValueError(f"down={down} outside [1, {self.MAX_FACTOR}]")
        b = _real_taps(taps, self.MAX_TAPS, lambda t: design.resample_coeffs(up, down, t))
        if -(-len(b) // up) > self.MAX_PHASE_TAPS:
            raise ValueError(f"{len(b)} taps at up={up}: more than {self.MAX_PHASE_TAPS} taps per phase")
        self.nrows, self.up, self.down, self.taps, self.complex = nrows, up, down, b, bool(complex)
        self.elems = 2 if self.complex else 1
        self.step = down // int(np.gcd(up, down))       # a call's n is a multiple of this
        self.ctx = ctx if ctx is not None else _lib.get_context()
        self.lib = self.ctx.lib
        h = ctypes.c_void_p()
        check(self.lib.sdr_rsmp_create(self.ctx.handle, nrows, self.elems, f64p(b), len(b), up, down, ctypes.byref(h)),
              "sdr_rsmp_create")
        self.handle = h

    def out_len(self, n: int) -> int:
        """Outputs per row of a call of n samples per row (n up / down)."""
        n = int(n)
        if n < 1 or n % self.step:
            raise ValueError(f"n={n} must be >= 1 and a multiple of down/gcd(up, down)={self.step}")
        return n * self.up // self.down

    def process(self, x) -> np.ndarray:
        """(nrows, n) samples from the host -> (nrows, n up / down), synchronous (sdr_rsmp_run)."""
        x = np.ascontiguousarray(x, dtype=np.complex64 if self.complex else np.float32)
        if x.ndim != 2 or x.shape[0] != self.nrows:
            raise ValueError(f"expected an array of shape ({self.nrows}, n)")
        n = x.shape[1]
        mo = self.out_len(n)
        out = np.empty((self.nrows, mo), dtype=x.dtype)
        check(self.lib.sdr_rsmp_run(self.handle, x.ctypes.data, n, n, out.ctypes.data, mo), "sdr_rsmp_run")
        return out

    def process_dev(self, in_ptr: int, n: int, in_stride: int, out_ptr: int, out_stride: int):
        """n samples per row at device pointer in_ptr, rows in_stride samples apart -> n up / down
        samples per row at out_ptr, rows out_stride samples apart; async on the context stream."""
        n, in_stride, out_stride = int(n), int(in_stride), int(out_stride)
        mo = self.out_len(n)
        if in_stride < n or out_stride < mo:
            raise ValueError(f"in_stride={in_stride} < n={n} or out_stride={out_stride} < n up/down={mo}")
        check(self.lib.sdr_rsmp_process_dev(self.handle, in_ptr, n, in_stride, out_ptr, out_stride), "sdr_rsmp_process_dev")


def spectrum_rows(n: int, nfft: int, hop: int, navg: int):
    """(nseg, rows) of a Spectrum call of n samples: nseg = (n - nfft) // hop + 1 segments,
    rows = nseg // navg (navg = 0: one row of all of them).  Host arithmetic (sdr_spec_rows)."""
    n, nfft, hop, navg = int(n), int(nfft), int(hop), int(navg)
    if n < nfft:
        raise ValueError(f"n={n} < nfft={nfft}")
    nseg = (n - nfft) // hop + 1
    rows = nseg // navg if navg > 0 else 1
    if rows < 1:
        raise ValueError(f"n={n} yields {nseg} segments, no complete row of navg={navg}")
    return nseg, rows


class Spectrum(_LazyHandle):
    """The spectrum / waterfall of a wideband IQ capture on the GPU (sdr_spec, csrc/spectrum.hip):
    Welch periodogram rows of the buffer Channelizer / FilterBank read, in place -- which of the
    band's channels carry a station?  With segment s starting at sample s hop and window w,

        X_s[k]    = sum_{i < nfft} w[i] x[s hop + i] exp(-2 pi i k i / nfft)
        out[r][j] = (1 / (navg (sum w)^2)) sum_{s in [r navg, (r + 1) navg)} |X_s[k]|^2,  k = (j + nfft / 2) mod nfft

    linear power in float32, bin j centred on freqs_hz[j] = (j - nfft / 2) fs / nfft (ascending, as
    np.fft.fftshift): scipy.signal.spectrogram(x, window=w, nperseg=nfft, noverlap=nfft - hop,
    detrend=False, return_onesided=False, scaling='spectrum', mode='psd') averaged over groups of
    navg columns and shifted.  navg = 0: one row of all segments.  Trailing segments that do not
    fill a row are ignored; nothing is carried between calls.

    nfft: a power of two in [64, 8192].  hop: 1 .. 2^24 (None: nfft), odd or even, larger than
    nfft for a sparse monitor.  window: a name for scipy.signal.get_window(name, nfft) (periodic),
    or nfft finite values of any sign whose sum is not zero.  scale = (sum w)^2: out * scale /
    (fs sum w^2) is the density.  The arguments are checked, and rows / freqs_hz / window / scale
    answer, before a context exists; the device object is made at the first call that needs it."""

    MIN_NFFT, MAX_NFFT, MAX_HOP = 64, 8192, 1 << 24              # include/sdr.h SDR_SPEC_*
    SPLIT_SEGS = 8                                               # a row of more segments may be summed in chunks (SDR_SPEC_SPLIT_SEGS)
    _prefix = "sdr_spec"

    def __init__(self, nfft: int, fs: float, hop=None, navg: int = 0, window="hann", iq_dtype=np.float32, ctx=None):
        self._set_geometry(nfft, fs, hop, navg, window)
        self.u8 = _is_u8(iq_dtype)
        self._ctx = ctx

    def _set_geometry(self, nfft, fs, hop, navg, window):
        """The checks and attributes Spectrum and RowSpectrum share (no context is touched)."""
        nfft, fs, navg = int(nfft), float(fs), int(navg)
        if not (np.isfinite(fs) and fs > 0):
            raise ValueError("fs must be positive")
        if not self.MIN_NFFT <= nfft <= self.MAX_NFFT or nfft & (nfft - 1):
            raise ValueError(f"nfft={nfft} must be a power of two in [{self.MIN_NFFT}, {self.MAX_NFFT}]")
        hop = nfft if hop is None else int(hop)
        if not 1 <= hop <= self.MAX_HOP:
            raise ValueError(f"hop={hop} outside [1, {self.MAX_HOP}]")
        if navg < 0:
            raise ValueError(f"navg={navg} must be 0 (one row) or >= 1")
        w = design.spectrum_window(window, nfft)
        self.nfft, self.fs, self.hop, self.navg, self.window = nfft, fs, hop, navg, w
        self.scale = float(np.sum(w)) ** 2

    @property
    def freqs_hz(self) -> np.ndarray:
        """The nfft bin centres, ascending: (j - nfft / 2) fs / nfft."""
        return (np.arange(self.nfft) - self.nfft // 2) * (self.fs / self.nfft)

    def rows(self, n: int):
        """(nseg, rows) of a call of n samples."""
        return spectrum_rows(n, self.nfft, self.hop, self.navg)

    def _create_args(self):
        return self.nfft, f64p(self.window), self.hop, self.navg, SDR_IQ_U8 if self.u8 else SDR_IQ_F32

    def process_dev(self, iq_ptr: int, n: int, out_ptr: int, out_stride=None) -> int:
        """n complex samples at device pointer iq_ptr -> rows of nfft float32 at out_ptr,
        out_stride floats apart (None: nfft; the floats between rows are not written); async on
        the context stream.  Returns the row count."""
        n = int(n)
        rows = self.rows(n)[1]
        out_stride = self.nfft if out_stride is None else int(out_stride)
        if out_stride < self.nfft:
            raise ValueError(f"out_stride={out_stride} < nfft={self.nfft}")
        self._do("process_dev", iq_ptr, n, out_ptr, out_stride)
        return rows

    def run(self, iq_host) -> np.ndarray:
        """n complex samples from the host (interleaved f32 / u8, or complex for an f32 object)
        -> float32[rows, nfft], synchronous (sdr_spec_run)."""
        iq = _interleaved_iq(iq_host, self.u8, "spectrum")
        n = iq.size // 2
        rows = self.rows(n)[1]
        out = np.empty((rows, self.nfft), dtype=np.float32)
        self._do("run", iq.ctypes.data, n, out.ctypes.data, self.nfft)
        return out


FoundChannels = collections.namedtuple("FoundChannels", "index freq_hz snr_db")


def find_channels(power_row, fs: float, spacing_hz: float, width_hz=None, min_snr_db: float = 10.0, offset_hz: float = 0.0,
                  isolated: bool = True) -> FoundChannels:
    """Which channels of a uniform grid carry a signal, from one Spectrum row (host, numpy).

    power_row: linear power of nbin bins in ascending order, bin i centred on (i - nbin / 2)
    fs / nbin.  Candidate centres are offset_hz + j spacing_hz for every integer j whose window
    [f - width / 2, f + width / 2) lies inside [-fs / 2, fs / 2); width_hz defaults to 0.8
    spacing_hz.  A candidate's power is the sum of the bins whose centres fall in its window; the
    noise floor per bin is the row's median -- valid while fewer than half of the bins are
    occupied, so a band more than half full of signals needs a floor from elsewhere -- and the
    SNR is the candidate's power over (median x bins in its window).  Kept: SNR >= min_snr_db,
    and with isolated=True a power not below that of either neighbouring candidate (an FM
    station's skirts reach into the adjacent slots of a 200 kHz grid).

    Returns (index, freq_hz, snr_db), arrays sorted by frequency; index is the signed j.  With
    spacing_hz == fs / nbins and offset_hz == 0 it is the signed bin numbers
    FilterBank(nbins, ..., bins=found.index) takes."""
    p = np.asarray(power_row, dtype=np.float64)
    fs, spacing, offset = float(fs), float(spacing_hz), float(offset_hz)
    if p.ndim != 1 or p.size < 2:
        raise ValueError("power_row: one row of at least two bins")
    if not (np.isfinite(fs) and fs > 0 and np.isfinite(spacing) and spacing > 0 and np.isfinite(offset)):
        raise ValueError("fs and spacing_hz must be positive, offset_hz finite")
    width = 0.8 * spacing if width_hz is None else float(width_hz)
    if not (np.isfinite(width) and width > 0):
        raise ValueError("width_hz must be positive")
    nbin = p.size
    centres = (np.arange(nbin) - nbin // 2) * (fs / nbin)
    jlo = int(np.ceil((-fs / 2 + width / 2 - offset) / spacing))
    jhi = int(np.floor((fs / 2 - width / 2 - offset) / spacing))
    j = np.arange(jlo, jhi + 1)
    j = j[(offset + j * spacing - width / 2 >= -fs / 2) & (offset + j * spacing + width / 2 <= fs / 2)]
    f = offset + j * spacing
    # bins [lo, hi) of every window: centres ascend, so the window is a slice of the prefix sums
    lo = np.searchsorted(centres, f - width / 2, side="left")
    hi = np.searchsorted(centres, f + width / 2, side="left")
    csum = np.r_[0.0, np.cumsum(p)]
    power = csum[hi] - csum[lo]
    floor = float(np.median(p))
    with np.errstate(divide="ignore", invalid="ignore"):
        snr = 10.0 * np.log10(power / (floor * (hi - lo)))
    keep = (hi > lo) & (snr >= float(min_snr_db))
    if isolated and len(j):
        left = np.r_[-np.inf, power[:-1]]
        right = np.r_[power[1:], -np.inf]
        keep &= (power >= left) & (power >= right)
    return FoundChannels(j[keep].astype(np.int64), f[keep], snr[keep])


class RowSpectrum(Spectrum):
    """The one-sided spectrum of `nrows` rows of real float32 samples on the GPU in one call
    (sdr_rspec, csrc/spectrum.hip) -- a Receiver's demodulated rows, read where the receiver left
    them: what does each stream hold after demodulation?  With segment s of row q starting at
    sample s hop and window w,

        X_qs[k]      = sum_{i < nfft} w[i] x_q[s hop + i] exp(-2 pi i k i / nfft),   k = 0 .. nfft / 2
        out[q][r][k] = (c_k / (navg (sum w)^2)) sum_{s in [r navg, (r + 1) navg)} |X_qs[k]|^2

    with c_0 = c_{nfft/2} = 1 and 2 otherwise: linear power in float32, bin k centred on
    freqs_hz[k] = k fs / nfft -- scipy.signal.spectrogram(x_q, window=w, nperseg=nfft,
    noverlap=nfft - hop, detrend=False, return_onesided=True, scaling='spectrum', mode='psd')
    averaged over groups of navg columns.  nfft, hop, navg, window, scale and rows(n) (per input
    row) are Spectrum's; nrows: 1 .. 65 535.  Nothing is carried between calls.  The arguments are
    checked, and the geometry answers, before a context exists.  mpx_quality reads the rows."""

    MAX_ROWS = 65535                                             # include/sdr.h SDR_RSPEC_MAX_ROWS
    _prefix = "sdr_rspec"

    def __init__(self, nrows: int, nfft: int, fs: float, hop=None, navg: int = 0, window="hann", ctx=None):
        nrows = int(nrows)
        if not 1 <= nrows <= self.MAX_ROWS:
            raise ValueError(f"nrows={nrows} outside [1, {self.MAX_ROWS}]")
        self._set_geometry(nfft, fs, hop, navg, window)
        self.nrows, self.nbins = nrows, self.nfft // 2 + 1
        self._ctx = ctx

    @property
    def freqs_hz(self) -> np.ndarray:
        """The nfft / 2 + 1 bin centres, 0 .. fs / 2: k fs / nfft."""
        return np.arange(self.nbins) * (self.fs / self.nfft)

    def _create_args(self):
        return self.nrows, self.nfft, f64p(self.window), self.hop, self.navg

    def process_dev(self, x_ptr: int, n: int, in_stride: int, out_ptr: int, out_stride=None) -> int:
        """n samples per row at device pointer x_ptr, rows in_stride floats apart -> per input row
        `rows` rows of nfft / 2 + 1 float32 at out_ptr, row (q, r) at (q rows + r) out_stride floats
        (None: nfft / 2 + 1; the floats between rows are not written); async on the context
        stream.  Returns rows."""
        n, in_stride = int(n), int(in_stride)
        rows = self.rows(n)[1]
        out_stride = self.nbins if out_stride is None else int(out_stride)
        if in_stride < n:
            raise ValueError(f"in_stride={in_stride} < n={n}")
        if out_stride < self.nbins:
            raise ValueError(f"out_stride={out_stride} < nfft/2+1={self.nbins}")
        self._do("process_dev", x_ptr, n, in_stride, out_ptr, out_stride)
        return rows

    def process_rx(self, receiver: "Receiver", out_ptr: int, name: str = "demod", out_stride=None) -> int:
        """The receiver's latest rows of output `name` (looked up at every call: a pipelined
        receiver alternates its row sets; call it before the receiver's next process_dev, which
        keeps the rows until this call has read them) -> out_ptr as process_dev.  Returns rows."""
        if receiver.S != self.nrows:
            raise ValueError(f"the receiver has {receiver.S} streams, the spectrum {self.nrows} rows")
        ptr, stride, n = receiver.output_ptr(name)
        return self.process_dev(ptr, n, stride, out_ptr, out_stride)

    def run(self, x_host) -> np.ndarray:
        """(nrows, n) real samples from the host -> float32[nrows, rows, nfft / 2 + 1], synchronous
        (sdr_rspec_run)."""
        x = np.ascontiguousarray(x_host, dtype=np.float32)
        if x.ndim != 2 or x.shape[0] != self.nrows:
            raise ValueError(f"expected an array of shape ({self.nrows}, n)")
        n = x.shape[1]
        rows = self.rows(n)[1]
        out = np.empty((self.nrows, rows, self.nbins), dtype=np.float32)
        self._do("run", x.ctypes.data, n, n, out.ctypes.data, self.nbins)
        return out


MpxQuality = collections.namedtuple("MpxQuality", "pilot_snr_db rds_snr_db noise_floor stereo rds")

MPX_PILOT_BAND, MPX_PILOT_GUARD = (18.5e3, 19.5e3), ((16e3, 18e3), (20e3, 22e3))
MPX_RDS_BAND, MPX_RDS_GUARD = (55e3, 59e3), ((60e3, 64e3),)


def mpx_quality(power, fs: float = 240e3, min_pilot_db: float = 15.0, min_rds_db: float = 6.0) -> MpxQuality:
    """A tuner's stereo lamp and signal meter from one-sided spectra of the FM multiplex (host,
    numpy): RowSpectrum rows of a Receiver's "demod" output, any shape (..., nfft / 2 + 1), bin k
    centred on k fs / nfft.

    A bin belongs to a band if its centre lies in the closed interval.  A subcarrier's ratio is
    sum(band) / (median(guard) x bins in band), in dB: the 19 kHz pilot in 18.5 - 19.5 kHz against
    the gaps 16 - 18 kHz and 20 - 22 kHz on either side of it (above the mono audio, below L-R),
    the RDS subcarrier in 55 - 59 kHz against 60 - 64 kHz.  noise_floor is the pilot guard's median
    (linear, per bin); stereo and rds are the ratios against min_pilot_db and min_rds_db.  All five
    have the shape power.shape[:-1].

    Needs fs / 2 > 64 kHz and bins no wider than 500 Hz (nfft >= 512 at 240 kHz): with wider bins
    the window's skirts of the audio and of the pilot fill the guard bands."""
    p = np.asarray(power, dtype=np.float64)
    fs = float(fs)
    if p.ndim < 1 or p.shape[-1] < 3:
        raise ValueError("power: rows of nfft / 2 + 1 bins")
    if not (np.isfinite(fs) and fs > 0):
        raise ValueError("fs must be positive")
    nfft = 2 * (p.shape[-1] - 1)
    if fs / 2 <= MPX_RDS_GUARD[-1][1]:
        raise ValueError(f"fs={fs}: the guard band up to {MPX_RDS_GUARD[-1][1]} Hz needs fs / 2 above it")
    if fs / nfft > 500.0:
        raise ValueError(f"bins of {fs / nfft:.1f} Hz ({p.shape[-1]} bins at fs={fs}) are wider than 500 Hz")
    f = np.arange(p.shape[-1]) * (fs / nfft)

    def ratio_db(band, guards):
        inb = (f >= band[0]) & (f <= band[1])
        ing = np.zeros(len(f), dtype=bool)
        for lo, hi in guards:
            ing |= (f >= lo) & (f <= hi)
        floor = np.median(p[..., ing], axis=-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            return 10.0 * np.log10(np.sum(p[..., inb], axis=-1) / (floor * np.count_nonzero(inb))), floor

    pilot, floor = ratio_db(MPX_PILOT_BAND, MPX_PILOT_GUARD)
    rds, _ = ratio_db(MPX_RDS_BAND, MPX_RDS_GUARD)
    return MpxQuality(pilot, rds, floor, pilot >= float(min_pilot_db), rds >= float(min_rds_db))


class _RmeterParamsC(ctypes.Structure):                          # include/sdr.h sdr_rmeter_params
    _fields_ = [("window", ctypes.c_int64), ("nbins", ctypes.c_int), ("scale", ctypes.c_float), ("limit", ctypes.c_float)]


class _RmeterRecordC(ctypes.Structure):                          # include/sdr.h sdr_rmeter_record
    _fields_ = [(k, {np.int64: ctypes.c_int64, np.float64: ctypes.c_double, np.float32: ctypes.c_float}[rowmeter.field_dtype(k)])
                for k in rowmeter.FIELDS]


class RowMeter(_Timed, _LazyHandle):
    """The modulation meter of `nstreams` rows of real float32 samples on the GPU (sdr_rmeter,
    csrc/rmeter.hip) -- a Receiver's "demod" or audio rows, read where the receiver left them.  Per
    stream and carried from call to call: the call's and the totals' finite / non-finite / over-limit
    counts, max, min, float64 sum and sum of squares, and the histogram (`nbins` bins, `scale` bins
    per unit of the row) of the half-spans (max - min) / 2 of consecutive windows of `window`
    samples, cut across calls by a 64-bit stream position.  Two launches per call, nothing returns to
    the host until records(), hist() or windows() is asked; the same calls give the same bits.

    The rule is rtsdr.RowMeterModel's (rowmeter.py): integers, peaks, histogram and windows equal it
    exactly, the float64 sums within the summation bound.  modulation_report reads a record.  The
    arguments are checked before a context exists; the device object is made at the first call that
    needs it."""

    CHUNK, SEG = _lib.SDR_RMETER_CHUNK, _lib.SDR_RMETER_SEG      # a window from SEG samples on is cut into chunks of at most CHUNK
    MAX_N = rowmeter.MAX_N
    _prefix = "sdr_rmeter"
    _STAGES = ("reduce", "fold")                                 # stage_ms: the last call's two launches

    def __init__(self, nstreams: int, window: int, nbins: int = 128, scale: float = 1.0, limit: float = np.inf, ctx=None):
        self.nstreams, self.window, self.nbins, self.scale, self.limit = rowmeter.check_params(nstreams, window, nbins, scale, limit)
        self._ctx = ctx

    def _create_args(self):
        return self.nstreams, ctypes.byref(_RmeterParamsC(self.window, self.nbins, float(self.scale), float(self.limit)))

    def process_dev(self, ptr: int, stride: int, n: int):
        """n samples per row at device pointer ptr, rows stride floats apart (the floats between rows
        are never read; any 4-byte alignment); async on the context stream."""
        ptr, stride, n = int(ptr or 0), int(stride), int(n)
        if not ptr:
            raise ValueError("ptr is NULL")
        if not 1 <= n <= self.MAX_N:
            raise ValueError(f"n={n} outside [1, 2^31 - 1]")
        if self.nstreams > 1 and stride < n:
            raise ValueError(f"stride={stride} < n={n}")
        if ptr % 4:
            raise ValueError("ptr must be aligned to 4 B")
        self._do("process_dev", ptr, stride, n)

    def process_rx(self, receiver: "Receiver", name: str = "demod"):
        """The receiver's latest rows of output `name`, read in place (looked up at every call: a
        pipelined receiver alternates its row sets; call it before the receiver's next process_dev,
        which keeps the rows until this call has read them)."""
        if receiver.S != self.nstreams:
            raise ValueError(f"the receiver has {receiver.S} streams, the meter {self.nstreams}")
        ptr, stride, n = receiver.output_ptr(name)
        self.process_dev(ptr, stride, n)

    def run(self, rows_host):
        """(nstreams, n) real samples from the host; synchronous (sdr_rmeter_run)."""
        x = np.ascontiguousarray(rowmeter.as_rows(rows_host, self.nstreams))
        self._do("run", x.ctypes.data, x.shape[1], x.shape[1])

    def records(self) -> "rowmeter.RowMeterRecord":
        """The state after the latest call, an array entry per stream (sdr_rmeter_records; synchronises)."""
        raw = (_RmeterRecordC * self.nstreams)()
        self._do("records", ctypes.byref(raw))
        return rowmeter.RowMeterRecord(*(np.array([getattr(r, k) for r in raw], dtype=rowmeter.field_dtype(k)) for k in rowmeter.FIELDS))

    def hist(self) -> np.ndarray:
        """uint64[nstreams, nbins] (sdr_rmeter_hist; synchronises)."""
        out = np.empty((self.nstreams, self.nbins), dtype=np.uint64)
        self._do("hist", out.ctypes.data)
        return out

    def windows(self) -> np.ndarray:
        """float32[nstreams, windows, 2]: (min, max) of the windows the latest call completed, in
        order; (+inf, -inf) for one without a finite sample (sdr_rmeter_windows; synchronises)."""
        counts = np.zeros(self.nstreams, dtype=np.int64)
        self._do("windows", None, 0, counts.ctypes.data)
        out = np.empty((self.nstreams, int(counts[0]), 2), dtype=np.float32)
        if out.size:
            self._do("windows", out.ctypes.data, out.shape[1], None)
        return out

    def state_ptr(self):
        """(record pointer, histogram pointer): the device arrays of struct sdr_rmeter_record [nstreams]
        and uint64 [nstreams][nbins] (sdr_rmeter_state_dev)."""
        return self._ptr_out("state_dev", 2)

    def reset(self):
        """Zero the records, the histogram and the stream position (async)."""
        self._do("reset")


class RowSos(_Timed, _LazyHandle):
    """A cascade of 1 .. 4 second-order sections on `nrows` rows of real float32 samples on the GPU
    (sdr_sos, csrc/sos.hip): scipy.signal.sosfilt(sos, x, zi) per row in float64, rounded once to
    float32, the state (scipy's zi / zf, [nrows, K, 2] float64) carried on the device from call to
    call.  sos: [K, 6] with a0 == 1 and every pole inside the unit circle (design.pilot_notch_sos,
    design.k_weighting_sos, scipy.signal.ellip / butter(..., output="sos")).  Three launches per
    call, one for rows of up to 2048 samples; the same calls give the same bits.  The rule is
    rtsdr.sos_model.  The arguments are checked before a context exists; the device object is made
    at the first call that needs it."""

    TILE, MAX_SECTIONS = _lib.SDR_SOS_TILE, _lib.SDR_SOS_MAX_SECTIONS
    MAX_N = sosfilter.MAX_N
    _prefix = "sdr_sos"
    _STAGES = ("reduce", "carry", "apply")                        # stage_ms: the last call's launches

    def __init__(self, nrows: int, sos, ctx=None):
        self.nrows, self.sos = sosfilter.check_rows_count(nrows), sosfilter.check_sos(sos)
        self.K = self.sos.shape[0]
        self._ctx = ctx

    def _create_args(self):
        return self.nrows, f64p(self.sos), self.K

    def process_dev(self, x_ptr: int, x_stride: int, y_ptr: int, y_stride: int, n: int):
        """n samples per row at device pointer x_ptr, rows x_stride floats apart, to y_ptr (y_stride
        apart): any 4-byte alignment, the floats between rows are never touched; y_ptr == x_ptr
        filters in place; y_ptr 0 / None stores nothing and only advances the state.  Async on the
        context stream."""
        x_ptr, y_ptr, x_stride, y_stride, n = int(x_ptr or 0), int(y_ptr or 0), int(x_stride), int(y_stride), int(n)
        if not x_ptr:
            raise ValueError("x_ptr is NULL")
        if not 1 <= n <= self.MAX_N:
            raise ValueError(f"n={n} outside [1, 2^31 - 1]")
        if x_stride < n or (y_ptr and y_stride < n):
            raise ValueError(f"stride ({x_stride}, {y_stride}) < n={n}")
        if x_ptr % 4 or y_ptr % 4:
            raise ValueError("x_ptr and y_ptr must be aligned to 4 B")
        self._do("process_dev", x_ptr, x_stride, y_ptr or None, y_stride, n)

    def process_rx(self, receiver: "Receiver", name: str, out_ptr=None):
        """The receiver's latest rows of output `name` (looked up at every call), filtered in place,
        or into out_ptr -- rows the same stride apart -- which leaves the receiver's rows as they are.
        Call it before the receiver's next process_dev, which keeps the rows until this call is done."""
        if receiver.S != self.nrows:
            raise ValueError(f"the receiver has {receiver.S} streams, the filter {self.nrows} rows")
        ptr, stride, n = receiver.output_ptr(name)
        self.process_dev(ptr, stride, ptr if out_ptr is None else out_ptr, stride, n)

    def run(self, rows_host) -> np.ndarray:
        """(nrows, n) real samples from the host to float32 (nrows, n); synchronous (sdr_sos_run)."""
        x = np.ascontiguousarray(sosfilter.as_rows(rows_host, self.nrows))
        y = np.empty_like(x)
        self._do("run", x.ctypes.data, y.ctypes.data, x.shape[1], x.shape[1])
        return y

    def state(self) -> np.ndarray:
        """float64 [nrows, K, 2]: scipy's zf after the latest call (sdr_sos_state; synchronises)."""
        z = np.empty((self.nrows, self.K, 2))
        self._do("state", z.ctypes.data)
        return z

    def set_state(self, z):
        """The state the next call starts from: float64 [nrows, K, 2], scipy's zi (synchronises)."""
        z = np.ascontiguousarray(z, dtype=np.float64)
        if z.shape != (self.nrows, self.K, 2):
            raise ValueError(f"state must be ({self.nrows}, {self.K}, 2), not {z.shape}")
        self._do("set_state", z.ctypes.data)

    def reset(self):
        """Zero state (async)."""
        self._do("reset")


class _LoudParamsC(ctypes.Structure):                            # include/sdr.h sdr_loud_params
    _fields_ = [("segment", ctypes.c_int64), ("cap", ctypes.c_int), ("reference", ctypes.c_double)]


class LoudnessMeter(_Timed, _LazyHandle):
    """Programme loudness of `nstreams` audio streams of 1 or 2 channels on the GPU (sdr_loud,
    csrc/sos.hip), read from a Receiver's 48 kHz audio rows where it left them: every row through
    the two K-weighting sections of ITU-R BS.1770 with carried state, divided by `reference` (the row
    amplitude of PCM full scale: the output stage writes int16(x * 16384), so 2.0), and the float64
    sum of squares of every completed segment of `segment` samples (4800: 100 ms) of stream
    position, the latest `cap` of them kept per stream and channel.  Four launches per call, nothing
    returns to the host until segments() or report() is asked.  The rule is rtsdr.LoudnessModel;
    report() is rtsdr.loudness_report of the kept segments: momentary, short-term and gated
    integrated loudness in LUFS (the default cap holds 409.6 s).  The arguments are checked before
    a context exists."""

    MAX_N = sosfilter.MAX_N
    _prefix = "sdr_loud"
    _STAGES = ("reduce", "carry", "apply", "fold")

    def __init__(self, nstreams: int, channels: int = 2, segment: int = 4800, cap: int = 4096, reference: float = 2.0, ctx=None):
        self.nstreams, self.channels, self.segment, self.cap, self.reference = sosfilter.check_loudness_params(nstreams, channels, segment, cap,
                                                                                                              reference)
        self._ctx = ctx

    def _create_args(self):
        return self.nstreams, self.channels, ctypes.byref(_LoudParamsC(self.segment, self.cap, self.reference))

    def process_dev(self, ch0_ptr: int, ch1_ptr: int, stride: int, n: int):
        """n samples per row of each channel at device pointers ch0_ptr and ch1_ptr (0 / None with one
        channel), rows stride floats apart, any 4-byte alignment; async on the context stream."""
        p0, p1, stride, n = int(ch0_ptr or 0), int(ch1_ptr or 0), int(stride), int(n)
        if not p0 or bool(p1) != (self.channels == 2):
            raise ValueError(f"{self.channels} channel(s): ch0_ptr must be given, ch1_ptr with two channels only")
        if not 1 <= n <= self.MAX_N:
            raise ValueError(f"n={n} outside [1, 2^31 - 1]")
        if stride < n:
            raise ValueError(f"stride={stride} < n={n}")
        if p0 % 4 or p1 % 4:
            raise ValueError("the row pointers must be aligned to 4 B")
        self._do("process_dev", p0, p1 or None, stride, n)

    def process_rx(self, receiver: "Receiver", names=None):
        """The receiver's latest rows of the outputs `names`, one per channel, read in place (None:
        receiver.loudness_rows(), ("left_de", "right_de") of a stereo receiver with de-emphasis).  Call
        it before the receiver's next process_dev, which keeps the rows until this call has read them."""
        if receiver.S != self.nstreams:
            raise ValueError(f"the receiver has {receiver.S} streams, the meter {self.nstreams}")
        names = receiver.loudness_rows() if names is None else tuple(names)
        if len(names) != self.channels:
            raise ValueError(f"{len(names)} outputs for {self.channels} channel(s)")
        rows = [receiver.output_ptr(k) for k in names]
        if any(r[1:] != rows[0][1:] for r in rows):
            raise ValueError("the channels' rows differ in stride or length")
        self.process_dev(rows[0][0], rows[1][0] if self.channels == 2 else None, rows[0][1], rows[0][2])

    def run(self, rows_host):
        """A list of `channels` arrays (nstreams, n) from the host; synchronous (sdr_loud_run)."""
        if len(rows_host) != self.channels:
            raise ValueError(f"{len(rows_host)} row sets for {self.channels} channel(s)")
        xs = [np.ascontiguousarray(sosfilter.as_rows(r, self.nstreams)) for r in rows_host]
        if any(x.shape != xs[0].shape for x in xs):
            raise ValueError("the channels' rows differ in length")
        self._do("run", xs[0].ctypes.data, xs[1].ctypes.data if self.channels == 2 else None, xs[0].shape[1], xs[0].shape[1])

    def segments(self):
        """(first, energies): float64 [nstreams, channels, count], the latest min(cap, completed)
        segment energies in order, and the stream index of the first (sdr_loud_segments; synchronises)."""
        buf = np.empty((self.nstreams, self.channels, self.cap))
        first, count = ctypes.c_int64(), ctypes.c_int64()
        self._do("segments", buf.ctypes.data, ctypes.byref(first), ctypes.byref(count))
        return first.value, np.ascontiguousarray(buf[:, :, :count.value])

    def report(self) -> "sosfilter.LoudnessReport":
        """rtsdr.loudness_report of the kept segments (a segment must be 100 ms of 48 kHz: 4800)."""
        return sosfilter.loudness_report(self.segments()[1], self.segment)

    def loudness_range(self) -> "truepeak.LoudnessRange":
        """rtsdr.loudness_range (EBU Tech 3342) of the kept segments (a segment must be 100 ms of 48 kHz: 4800)."""
        return truepeak.loudness_range(self.segments()[1], self.segment)

    def state_ptr(self):
        """(ring pointer, open pointer): the device arrays float64 [nstreams][channels][cap] (segment g
        at g % cap) and [nstreams][channels] (sdr_loud_state_dev)."""
        return self._ptr_out("state_dev", 2)

    def reset(self):
        """Zero the filter states, the segments and the stream position (async)."""
        self._do("reset")


class _TpeakParamsC(ctypes.Structure):                           # include/sdr.h sdr_tpeak_params
    _fields_ = [("up", ctypes.c_int), ("taps", ctypes.c_int), ("h", ctypes.c_void_p), ("segment", ctypes.c_int64), ("cap", ctypes.c_int)]


class _TpeakRecordC(ctypes.Structure):                           # include/sdr.h sdr_tpeak_record
    _fields_ = [(k, ctypes.c_int64 if truepeak.field_dtype(k) is np.int64 else ctypes.c_double) for k in truepeak.FIELDS]


class TruePeakMeter(_Timed, _LazyHandle):
    """The true peak of `nstreams` audio streams of 1 or 2 channels on the GPU (sdr_tpeak,
    csrc/tpeak.hip), read from a Receiver's 48 kHz audio rows where it left them: per input sample
    the `up` values of a polyphase interpolator `taps` ([up, taps] float32; None: the 4 x 12 table
    of ITU-R BS.1770-4 annex 2, design.true_peak_fir) as float64 chains in registers, of which only
    maxima are kept -- per completed segment of `segment` samples (4800: 100 ms) of stream position
    the true peak and the sample peak, the latest `cap` of them per stream and channel, and a record
    of the call and the totals.  Two launches per call, nothing returns to the host until records(),
    segments() or report() is asked.  The rule is rtsdr.TruePeakModel, which the device equals bit
    for bit; report() is rtsdr.true_peak_report in dBTP relative to `reference`, the row amplitude
    of PCM full scale (the output stage writes int16(x * 16384), so 2.0).  The arguments are checked
    before a context exists."""

    MAX_N = sosfilter.MAX_N
    _prefix = "sdr_tpeak"
    _STAGES = ("reduce", "fold")                                  # stage_ms: the last call's two launches

    def __init__(self, nstreams: int, channels: int = 2, segment: int = 4800, cap: int = 4096, taps=None, reference: float = 2.0, ctx=None):
        self.nstreams, self.channels, self.segment, self.cap, self.taps = truepeak.check_params(nstreams, channels, segment, cap, taps)
        self.reference = float(reference)
        if not (np.isfinite(self.reference) and self.reference > 0):
            raise ValueError(f"reference={reference} is not finite and positive")
        self._ctx = ctx

    def _create_args(self):
        up, taps = self.taps.shape
        return self.nstreams, self.channels, ctypes.byref(_TpeakParamsC(up, taps, self.taps.ctypes.data, self.segment, self.cap))

    def process_dev(self, ch0_ptr: int, ch1_ptr: int, stride: int, n: int):
        """n samples per row of each channel at device pointers ch0_ptr and ch1_ptr (0 / None with one
        channel), rows stride floats apart, any 4-byte alignment; async on the context stream."""
        p0, p1, stride, n = int(ch0_ptr or 0), int(ch1_ptr or 0), int(stride), int(n)
        if not p0 or bool(p1) != (self.channels == 2):
            raise ValueError(f"{self.channels} channel(s): ch0_ptr must be given, ch1_ptr with two channels only")
        if not 1 <= n <= self.MAX_N:
            raise ValueError(f"n={n} outside [1, 2^31 - 1]")
        if stride < n:
            raise ValueError(f"stride={stride} < n={n}")
        if p0 % 4 or p1 % 4:
            raise ValueError("the row pointers must be aligned to 4 B")
        self._do("process_dev", p0, p1 or None, stride, n)

    def process_rx(self, receiver: "Receiver", names=None):
        """The receiver's latest rows of the outputs `names`, one per channel, read in place (None:
        receiver.loudness_rows()).  Call it before the receiver's next process_dev, which keeps the
        rows until this call has read them."""
        if receiver.S != self.nstreams:
            raise ValueError(f"the receiver has {receiver.S} streams, the meter {self.nstreams}")
        names = receiver.loudness_rows() if names is None else tuple(names)
        if len(names) != self.channels:
            raise ValueError(f"{len(names)} outputs for {self.channels} channel(s)")
        rows = [receiver.output_ptr(k) for k in names]
        if any(r[1:] != rows[0][1:] for r in rows):
            raise ValueError("the channels' rows differ in stride or length")
        self.process_dev(rows[0][0], rows[1][0] if self.channels == 2 else None, rows[0][1], rows[0][2])

    def run(self, rows_host):
        """A list of `channels` arrays (nstreams, n) from the host; synchronous (sdr_tpeak_run)."""
        if len(rows_host) != self.channels:
            raise ValueError(f"{len(rows_host)} row sets for {self.channels} channel(s)")
        xs = [np.ascontiguousarray(sosfilter.as_rows(r, self.nstreams)) for r in rows_host]
        if any(x.shape != xs[0].shape for x in xs):
            raise ValueError("the channels' rows differ in length")
        self._do("run", xs[0].ctypes.data, xs[1].ctypes.data if self.channels == 2 else None, xs[0].shape[1], xs[0].shape[1])

    def records(self) -> "truepeak.TruePeakRecord":
        """The state after the latest call, every field [nstreams, channels] (sdr_tpeak_records; synchronises)."""
        raw = (_TpeakRecordC * (self.nstreams * self.channels))()
        self._do("records", ctypes.byref(raw))
        return truepeak.TruePeakRecord(*(np.array([getattr(r, k) for r in raw], dtype=truepeak.field_dtype(k)).reshape(self.nstreams, self.channels)
                                         for k in truepeak.FIELDS))

    def segments(self):
        """(first, peaks, sample_peaks): float64 [nstreams, channels, count] each, the latest min(cap,
        completed) segments' true and sample peaks in order, and the stream index of the first
        (sdr_tpeak_segments; synchronises)."""
        pk, sp = (np.empty((self.nstreams, self.channels, self.cap)) for _ in range(2))
        first, count = ctypes.c_int64(), ctypes.c_int64()
        self._do("segments", pk.ctypes.data, sp.ctypes.data, ctypes.byref(first), ctypes.byref(count))
        return first.value, np.ascontiguousarray(pk[:, :, :count.value]), np.ascontiguousarray(sp[:, :, :count.value])

    def report(self) -> "truepeak.TruePeakReport":
        """rtsdr.true_peak_report of the kept segments and the records, relative to `reference`."""
        _, pk, sp = self.segments()
        return truepeak.true_peak_report(pk, sp, self.records(), self.reference)

    def state_ptr(self):
        """(true-peak ring, sample-peak ring, records): the device arrays float64 [nstreams][channels][cap]
        (segment g at g % cap) twice and struct sdr_tpeak_record [nstreams][channels] (sdr_tpeak_state_dev)."""
        return self._ptr_out("state_dev", 3)

    def reset(self):
        """Zero the history, the segments, the records and the stream position (async)."""
        self._do("reset")


class _BlendParamsC(ctypes.Structure):                           # include/sdr.h sdr_blend_params
    _fields_ = [(n, ctypes.c_double) for n in ("blend_lo_db", "blend_hi_db", "mute_lo_db", "mute_hi_db", "attack", "release")]


class BlendParams(collections.namedtuple("BlendParams", "blend_lo_db blend_hi_db mute_lo_db mute_hi_db attack release")):
    """The gain control's parameters (sdr_blend_params).  The stereo gain goes from 0 at a pilot
    ratio of blend_lo_db (15: mpx_quality's lamp threshold) to 1 at blend_hi_db; the mute gain from
    1 at a noise floor of mute_lo_db (10 log10 of mpx_quality's noise_floor) to 0 at mute_hi_db,
    both +inf (the default): mute off.  attack / release: the share of the way to its target a
    gain moves per update when the target is below / not below it, in (0, 1]."""
    __slots__ = ()

    def __new__(cls, blend_lo_db=15.0, blend_hi_db=25.0, mute_lo_db=np.inf, mute_hi_db=np.inf, attack=1.0, release=0.25):
        p = super().__new__(cls, *(float(v) for v in (blend_lo_db, blend_hi_db, mute_lo_db, mute_hi_db, attack, release)))
        if not (np.isfinite(p.blend_lo_db) and np.isfinite(p.blend_hi_db) and p.blend_lo_db < p.blend_hi_db):
            raise ValueError(f"blend limits {p.blend_lo_db}, {p.blend_hi_db} dB: finite, lo < hi")
        if not (0.0 < p.attack <= 1.0 and 0.0 < p.release <= 1.0):
            raise ValueError(f"attack {p.attack}, release {p.release} outside (0, 1]")
        if not (p.mute_on and p.mute_lo_db < p.mute_hi_db) and not (p.mute_lo_db == np.inf and p.mute_hi_db == np.inf):
            raise ValueError(f"mute limits {p.mute_lo_db}, {p.mute_hi_db} dB: both +inf (off), or finite with lo < hi")
        return p

    @property
    def mute_on(self) -> bool:
        return bool(np.isfinite(self.mute_lo_db) and np.isfinite(self.mute_hi_db))

    def _c(self):
        return _BlendParamsC(*self)


def _blend_params(params):
    """A `params` argument: None (the defaults), a BlendParams, or the six values of one."""
    if params is None or params is True:
        return BlendParams()
    return params if isinstance(params, BlendParams) else BlendParams(*params)


def _check_mpx_bins(nbins: int, fs: float):
    """mpx_quality's conditions on a spectrum of nbins bins at fs, and the gain control's cap on
    its guard bands (SDR_BLEND_MAX_GUARD bins each)."""
    nbins, fs = int(nbins), float(fs)
    if nbins < 3:
        raise ValueError("power: rows of nfft / 2 + 1 bins")
    if not (np.isfinite(fs) and fs > 0):
        raise ValueError("fs must be positive")
    nfft = 2 * (nbins - 1)
    if fs / 2 <= MPX_RDS_GUARD[-1][1]:
        raise ValueError(f"fs={fs}: the guard band up to {MPX_RDS_GUARD[-1][1]} Hz needs fs / 2 above it")
    if fs / nfft > 500.0:
        raise ValueError(f"bins of {fs / nfft:.1f} Hz ({nbins} bins at fs={fs}) are wider than 500 Hz")
    f = np.arange(nbins) * (fs / nfft)
    for guards in (MPX_PILOT_GUARD, MPX_RDS_GUARD):
        if sum(np.count_nonzero((f >= lo) & (f <= hi)) for lo, hi in guards) > BlendControl.MAX_GUARD:
            raise ValueError(f"{nbins} bins at fs={fs}: a guard of more than {BlendControl.MAX_GUARD} bins")


BlendState = collections.namedtuple("BlendState", "pilot_snr_db rds_snr_db noise_floor stereo_gain mute_gain")


class BlendControl(_LazyHandle):
    """Stereo blend and noise mute gains of `nstreams` streams from their multiplex spectra, on the
    GPU (sdr_blend, csrc/blend.hip): update_dev reads one RowSpectrum row (navg=0) per stream,
    computes mpx_quality's pilot and RDS ratios and noise floor in f64, and moves each stream's
    gains towards

        target_g = clip((pilot_snr_db - blend_lo_db) / (blend_hi_db - blend_lo_db), 0, 1)
        target_m = clip((mute_hi_db - 10 log10(noise_floor)) / (mute_hi_db - mute_lo_db), 0, 1)

    by cur += k (target - cur), k = attack when the target is below cur, else release (a NaN gives
    target 0; mute off: m = 1).  One launch, one wave per stream, nothing comes back to the host;
    audio_blend_dev ramps the rows from the previous gains to the new ones (gains_ptr).  After
    creation and reset(): g = 0 (mono until a pilot has been seen), m = 0 with mute on, else 1.
    The arguments are checked before a context exists."""

    MAX_GUARD = 1024                                             # include/sdr.h SDR_BLEND_MAX_GUARD
    NSTATE = 8                                                   # SDR_BLEND_NSTATE
    _prefix = "sdr_blend"

    def __init__(self, nstreams: int, params=None, ctx=None):
        nstreams = int(nstreams)
        if not 1 <= nstreams <= 65535:
            raise ValueError(f"nstreams={nstreams} outside [1, 65535]")
        self.nstreams, self.params = nstreams, _blend_params(params)
        self._ctx = ctx

    def _create_args(self):
        return self.nstreams, ctypes.byref(self.params._c())

    def update_dev(self, power_ptr: int, nbins: int, stride: int, fs: float):
        """One update from nstreams rows of nbins float32 power bins at device pointer power_ptr,
        `stride` floats apart (bin k centred on k fs / (2 (nbins - 1))); async on the context stream."""
        nbins, stride, fs = int(nbins), int(stride), float(fs)
        if not power_ptr:
            raise ValueError("power_ptr is NULL")
        _check_mpx_bins(nbins, fs)
        if stride < nbins:
            raise ValueError(f"stride={stride} < nbins={nbins}")
        self._do("update_dev", power_ptr, nbins, stride, fs)

    def raw_state(self) -> np.ndarray:
        """(nstreams, 8) float64: pilot_db, rds_db, noise_floor, g_prev, g, m_prev, m, n_updates
        (sdr_blend_state; synchronises)."""
        out = np.empty((self.nstreams, self.NSTATE))
        self._do("state", f64p(out))
        return out

    def state(self) -> BlendState:
        """The latest update's quality and the gains now in force, arrays of nstreams values."""
        return _blend_state(self.raw_state())

    @property
    def gains_ptr(self) -> int:
        """The device array (nstreams, 4) float64 {g_prev, g, m_prev, m} (sdr_blend_gains_dev)."""
        return self._ptr_out("gains_dev")

    def reset(self):
        """Back to the state after creation (async)."""
        self._do("reset")


def _blend_state(raw) -> BlendState:
    return BlendState(raw[:, 0].copy(), raw[:, 1].copy(), raw[:, 2].copy(), raw[:, 4].copy(), raw[:, 6].copy())
