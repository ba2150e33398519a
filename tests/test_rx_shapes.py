"""The block receiver (sdr_rx, csrc/rx.hip and its stage kernels, csrc/rx_stage.hip) at ragged block
lengths and with non-default filters and decimations.

Every other receiver test that meets the oracle uses blocks that are whole tiles of every kernel
(B = 153 600 and multiples, 51 200).  Here the last window / tile is partial, a second stream's row
lies directly behind a partial window, a block is shorter than taps - 1, and the plan of rx_plan
(span, codes, cres, tiles_ok, lng, th32) is walked through the corners no other test reaches.

The reference is tests/rx_replay.py: per output row the f64 oracle primitive of that stage alone on
the device's own input rows, every state carried in f64, so that every sample of every block --
the first taps - 1 outputs and the last partial tile included -- compares at the bounds the suite
already asserts at the round shapes (no new number: DEMOD_*, AUDIO_*, RDS_TOL, NCO_REPLAY and the
bounds of test_span's _check_oracle_block (a) and _check_mixers; left / right alone is derived).
"""
import functools

import numpy as np
import pytest
from scipy import signal

import rx_replay
from conftest import LONG_PB, long_blocks, maxabs, rms
from test_receiver import AUDIO_MAX, AUDIO_RMS, RDS_TOL
from test_span import NCO_NAMES, NCO_REPLAY

gpu = pytest.mark.gpu

# ---- the library's constants the expectations are derived from (copied, as conftest does LONG_PB) ----
SDR_PLL_BLOCK_MAX = 16385          # csrc/sdr_launch.h:115: the longest per-block solve; beyond it a long call
MM_WT, MM_MIN_WIN = 1024, 32       # csrc/rx_stage.hip:451-453: outputs per matrix-core window; windows for a span
TH32_LINE = 32                     # csrc/sdr_nco.h:127: compact phase rows need pseudo-blocks of whole lines
CODE_TAPS = (101, 151)             # csrc/rx_stage.hip:1095-1098 mmable(): the tap counts the matrix cores take
CR_TO = 1216                       # csrc/rx_stage.hip:1311: outputs per tile of the composite RDS resampler

DEMOD_RMS, DEMOD_MAX = 1e-6, 1e-5  # tests/test_receiver.py (module docstring and :68)
PEAK_MAX = {"bpf_recovery": 2e-6, "bpf_extraction": 4e-6,      # test_span._check_oracle_block (a)
            "stereo": 1e-6, "lpf_i": 2e-6, "lpf_q": 1e-6}      # test_span._check_mixers
LR_ROUND = 1.2e-7                  # two f32 roundings (2 x 2^-24) of the larger operand of (audio +- stereo) / 2
PHASE_TOL, PLL_STATE_TOL = 1e-5, 1e-6   # test_receiver_carried_state_matches_oracle; test_fm_pll_zero_and_signed_inputs

ALL = ["demod", "audio", "stereo", "left", "right", "bpf_recovery", "nco", "bpf_extraction"] + list(RDS_TOL)
# test_span.py's lean keep set (_check_keep_lean)
LEAN = [nm for nm in ALL if nm not in NCO_NAMES + ("lpf_i", "lpf_q", "bpf_recovery", "pre_pll")]
NBLOCKS = 3


def is_span(M):
    """mm_span_ok (csrc/rx_stage.hip:1088), below its 2^28 limit"""
    return M >= MM_MIN_WIN * MM_WT and M % 4 == 0


def long_geom(M):
    """(long call?, pseudo-block length, pseudo-blocks): csrc/pll.hip long_n (:1892) and long_geom (:1906-1910)"""
    if M <= SDR_PLL_BLOCK_MAX:
        return False, M, 1
    k = -(-M // LONG_PB)
    return True, (LONG_PB if M - (k - 1) * LONG_PB >= 2 else -(-M // k)), k


# ---- the cases -------------------------------------------------------------------------------------
# section 2: default filters, u8.  (B, S): what it is the smallest case of
SHAPES = [
    (7, 1),            # M = 1 < 2: Q-form rows, NCO rows forced
    (1_003, 1),        # M = 101 < taps - 1: zf from old state plus new samples; A = 21, R = 24
    (16_007, 1),       # M = 1 601: `small` tiles, a partial tile everywhere, B % 10 != 0
    (163_850, 1),      # M = 16 385: the longest per-block solve
    (163_880, 1),      # M = 16 388: first long call, 2 pseudo-blocks, the last of 2 052; compact rows, VALU mixers
    (286_730, 1),      # M = 28 673: balanced pseudo-blocks of 9 558 (not whole lines): full rows in a long call
    (327_680, 1),      # M = 32 768: first span, 32 whole windows; A = 6 554 (M % 5 = 3), R = 7 783 (6 tiles + 487)
    (327_720, 2),      # M = 32 772: the 33rd window holds 4 outputs; a second stream's row behind it
    (327_700, 1),      # M = 32 770: beyond the span length but M % 4 != 0: VALU tiles, long call
    (329_995, 1),      # M = 33 000: span, last window of 232 outputs, B % 10 != 0
]
# section 3: name -> Receiver arguments that differ from the defaults, and the two block lengths
CONFIGS = {
    "taps101": (dict(stereo_taps=101, rds_taps=101), (16_007, 327_720)),
    "taps75": (dict(stereo_taps=75, rds_taps=75), (16_007, 327_720)),
    "audio_decim4": (dict(audio_decim=4), (16_007, 327_720)),
    "rf_decim8": (dict(rf_decim=8, rf_taps=51), (12_807, 262_176)),          # M = 1 601 and 32 772
}
# f32 / u8 blocks from device memory on the receiver's generic-FE branch (sdr_rx_process_dev: fast == false)
DEV_FEEDS = {
    "f32_pad1_S3": dict(dtype=np.float32, S=3, pad=1, lead=0, generic=False),   # iq_stride = B + 1: rows 16 B apart mod 16
    "f32_odd_stride_S3": dict(dtype=np.float32, S=3, pad=2, lead=0, generic=True),   # an odd iq_stride (B + 2)
    "f32_base_plus1": dict(dtype=np.float32, S=1, pad=0, lead=1, generic=True),      # base 8 B past a 16-B boundary
    "u8_base_plus2B": dict(dtype=np.uint8, S=1, pad=0, lead=1, generic=True),        # base 2 B past a 4-B boundary
    "u8_base_plus2B_S2": dict(dtype=np.uint8, S=2, pad=3, lead=1, generic=True),     # and a second row behind it
}


@functools.lru_cache(maxsize=None)
def _iq(n, seed, u8=True, fs=2.4e6):
    import rtsdr
    a = rtsdr.synth.fm_iq(n, seed=seed, fs=fs, dtype=np.uint8 if u8 else np.float32)
    a.setflags(write=False)
    return a


def _norm(blk):
    return (blk.astype(np.float64) - 128.0) / 128.0 if blk.dtype == np.uint8 else blk.astype(np.float64)


def _taps(oracle, rf_taps=151, stereo_taps=151, rds_taps=151, fs=2.4e6):
    """the receiver's filters from the oracle's designs (scipy.signal.firwin), never the library's;
    the RF low-pass (100 kHz, model/fmMonoBlock.py:43) designed at the capture rate fs"""
    rf = oracle.mono_coeffs(rf_taps, 151)[0] if fs == 2.4e6 else signal.firwin(rf_taps, 100e3 / (fs / 2), window="hann")
    audio = signal.firwin(151, 16e3 / 120e3, window="hann")
    pilot, band, slpf = oracle.stereo_coeffs(stereo_taps)
    co = oracle.rds_coeffs(rds_taps)
    return dict(rf=rf, audio=audio, pilot=pilot, stereo_bpf=band, stereo_lpf=slpf, rds_extract=co["extract"],
                rds_square=co["square"], rds_lpf=co["lpf"], rds_anti=co["anti_img"], rds_rrc=co["rrc"])


# ---- the comparison --------------------------------------------------------------------------------
def _shares(name, got, ref, dev):
    """the errors of one row of one block as shares of their bounds: [(which, error / bound)]"""
    em, er = maxabs(got, ref), rms(got, ref)
    peak = max(float(np.max(np.abs(ref))), 1e-3)
    if name == "demod":
        return [("rms", er / DEMOD_RMS), ("max", em / DEMOD_MAX)]
    if name == "audio":
        return [("rms", er / AUDIO_RMS), ("max", em / AUDIO_MAX)]
    if name in PEAK_MAX:
        return [("max", em / peak / PEAK_MAX[name])]
    if name in NCO_NAMES:
        return [("max", em / NCO_REPLAY)]
    if name in ("left", "right"):
        big = max(float(np.max(np.abs(dev["audio"]))), float(np.max(np.abs(dev["stereo"]))))
        # (both operands exactly zero -- a stream's first sample meets firwin's zero end tap -- bound 0: exact)
        return [("max", em / (LR_ROUND * big) if big > 0.0 else (0.0 if em == 0.0 else float("inf")))]
    tmax, trms = RDS_TOL[name]
    return [("max", em / peak / tmax), ("rms", er / peak / trms)]


def _expect_lengths(B, rf_decim, audio_decim):
    M, A, R = rx_replay.lengths(B, rf_decim, audio_decim)
    n = {nm: M for nm in ("demod", "bpf_recovery", "bpf_extraction", "extract", "pre_pll", "lpf_i", "lpf_q")}
    n.update({nm: M + 1 for nm in NCO_NAMES})
    n.update({nm: A for nm in ("audio", "stereo", "left", "right")})
    n.update({nm: R for nm in ("resample_i", "resample_q", "rrc_i", "rrc_q")})
    return M, n


class _HostFeed:
    """blocks from host arrays through Receiver.process (sdr_rx_run)"""

    def __init__(self, iq, B):
        self.iq, self.B = iq, B

    def block(self, k):
        return self.iq[:, 2 * k * self.B:2 * (k + 1) * self.B]

    def run(self, rx, k, names):
        return rx.process(self.block(k), fetch=names)

    def close(self):
        pass


class _DevFeed(_HostFeed):
    """blocks from device memory through Receiver.process_dev: rows B + pad complex samples apart,
    the base `lead` complex samples past an aligned address; everything around the rows is filled
    with values no sample takes (a read beyond a row's end shows in the outputs)"""

    def __init__(self, ctx, iq, B, pad, lead):
        from importlib import import_module
        _lib = import_module("real-time-software-defined-radio_amd._lib")
        super().__init__(iq, B)
        S = len(iq)
        self.stride = B + pad
        junk = 255 if iq.dtype == np.uint8 else 1e3
        self.bufs, self.ptrs = [], []
        for k in range(NBLOCKS):
            host = np.full(2 * (lead + S * self.stride + 64), junk, dtype=iq.dtype)
            for s in range(S):
                at = 2 * (lead + s * self.stride)
                host[at:at + 2 * B] = self.block(k)[s]
            d = _lib.DeviceBuffer.from_array(ctx, host)
            assert d.ptr % 256 == 0
            self.bufs.append(d)
            self.ptrs.append(d.ptr + 2 * lead * iq.dtype.itemsize)
        ctx.synchronize()

    def run(self, rx, k, names):
        rx.process_dev(self.ptrs[k], self.stride)
        return {nm: rx.output(nm) for nm in names}

    def close(self):
        for d in self.bufs:
            d.free()


def _check_case(sdr, gpu_ctx, oracle, B, S, seed0, kw=None, rf_taps=151, dev_feed=None, tag=""):
    """NBLOCKS consecutive blocks of S streams through a receiver that keeps every intermediate
    and through a lean one; see the tests below for what is asserted"""
    kw = dict(kw or {})
    dtype = dev_feed["dtype"] if dev_feed else np.uint8
    rf_decim, audio_decim = kw.get("rf_decim", 10), kw.get("audio_decim", 5)
    stereo_taps, rds_taps = kw.get("stereo_taps", 151), kw.get("rds_taps", 151)
    # the capture rate that puts the demodulated multiplex at the 240 kS/s the stage filters and the
    # PLLs are designed for (2.4 MS/s at the reference's decimation by 10)
    fs = 240e3 * rf_decim
    taps = _taps(oracle, rf_taps, stereo_taps, rds_taps, fs)
    if rf_taps != 151:
        kw["rf_coeff"] = taps["rf"]
    if audio_decim != 5:
        kw["audio_coeff"] = taps["audio"]
    kw.update(stereo=True, rds=True, iq_dtype=dtype)
    M, want_n = _expect_lengths(B, rf_decim, audio_decim)
    lng, pb, nb = long_geom(M)
    assert nb == long_blocks(M)
    span = is_span(M)
    codes = span and stereo_taps in CODE_TAPS and rds_taps in CODE_TAPS

    iq = np.stack([_iq(NBLOCKS * B, seed0 + s, dtype == np.uint8, fs) for s in range(S)])
    feed = _DevFeed(gpu_ctx, iq, B, dev_feed["pad"], dev_feed["lead"]) if dev_feed else _HostFeed(iq, B)
    full, lean = sdr.Receiver(S, B, **kw), sdr.Receiver(S, B, keep=LEAN, **kw)
    assert (full.M, full.A, full.R) == rx_replay.lengths(B, rf_decim, audio_decim)
    replay = rx_replay.Replay(oracle, S, taps, rf_decim, audio_decim)
    worst, fails = {}, []
    try:
        for k in range(NBLOCKS):
            for rx in (full, lean):
                gpu_ctx.pll_stats(reset=True)
                out = feed.run(rx, k, ALL if rx is full else LEAN)
                st = rx.pll_stats()
                # the PLL's path: one recurrence per pseudo-block, loop and stream; a long call's all
                # go through the long-call bookkeeping, a per-block call's none
                assert st["recurrences"] == 2 * S * nb, (k, st)
                assert st["long_guessed"] + st["long_chained"] == (2 * S * nb if lng else 0), (k, st)
                if rx is full:
                    got = out
            for nm in ALL:
                assert got[nm].shape == (S, want_n[nm]), (nm, got[nm].shape, want_n[nm])
            # the lean receiver: bit for bit what the full one gives, and no f32 PLL-input row
            # exactly where the PLLs read sign codes (a span with 101- / 151-tap loop filters)
            for nm in LEAN:
                assert np.array_equal(out[nm], got[nm]), (nm, k)
            if codes:
                with pytest.raises(ValueError, match="not materialised"):
                    lean.output("pre_pll")
            else:
                assert lean.output("pre_pll").shape == (S, M)
            ref = replay.block([_norm(feed.block(k)[s]) for s in range(S)], got)
            for nm in ALL:
                for s in range(S):
                    assert ref[nm][s].shape == got[nm][s].shape, (nm, s, k)
                    dev = {a: got[a][s] for a in ("audio", "stereo")}
                    for which, share in _shares(nm, got[nm][s], ref[nm][s], dev):
                        worst[nm] = max(worst.get(nm, 0.0), share)
                        if not share < 1.0:
                            fails.append((nm, which, f"{share:.3g}", "stream", s, "block", k))
        ph, ps, pr = full.state()
        for a, b in zip(lean.state(), (ph, ps, pr)):
            assert np.array_equal(a, b)
        rph, rps, rpr = replay.state()
        st_err = {"phase": maxabs(ph, rph) / PHASE_TOL, "pll_stereo": maxabs(ps, rps) / PLL_STATE_TOL,
                  "pll_rds": maxabs(pr, rpr) / PLL_STATE_TOL}
    finally:
        feed.close()
        full.close()
        lean.close()
    print(f"rx_shapes {tag} B={B} M={M} S={S} long={lng} pb={pb} nb={nb} span={span} codes={codes}: "
          f"worst error per row as a share of its bound:",
          {nm: f"{worst[nm]:.2f}" for nm in ALL}, "; carried states:", {a: f"{v:.2f}" for a, v in st_err.items()},
          f"; largest share {max(list(worst.values()) + list(st_err.values())):.2f}")
    assert not fails, fails
    for a, v in st_err.items():
        assert v < 1.0, (a, v)


# ---- section 2 -------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("B,S", SHAPES, ids=[f"B{b}" for b, _ in SHAPES])
def test_rx_shape_matches_stage_replay(sdr, gpu_ctx, oracle, B, S):
    """Default filters, u8 IQ, stereo + RDS, every intermediate kept, 3 consecutive blocks (the
    carried state crosses two ragged seams).  Every output row of every block against its stage's
    f64 replay on the device's own inputs (tests/rx_replay.py) at the suite's bounds; the output
    lengths; the carried demod phase and PLL states; the solver counters of the intended PLL path
    (per-block solve or long call, nb pseudo-blocks); a lean receiver (test_span's keep set) bit
    for bit equal, whose pre_pll row is absent exactly on spans."""
    _check_case(sdr, gpu_ctx, oracle, B, S, seed0=200, tag="default")


# ---- section 3 -------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name,big", [(n, b) for n in CONFIGS for b in (0, 1)],
                         ids=[f"{n}-{'span' if b else 'small'}" for n in CONFIGS for b in (0, 1)])
def test_rx_config_matches_stage_replay(sdr, gpu_ctx, oracle, name, big):
    """Non-default filters and decimations, each at a small ragged block and at the span length
    M = 32 772 (S = 1, otherwise as test_rx_shape_matches_stage_replay):
      taps101       the <101> kernels; no composite resampler (it needs 151 + 151 taps): the two-stage
                    D with JK_RESAMPLE, LPF and NCO rows forced
      taps75        rx_stage_kernel<0> for every stage filter; no sign codes at the span length (the
                    lean receiver's pre_pll is a row)
      audio_decim4  tiles_ok false: the stereo mixer reads NCO rows (PRE_MIX) and decimates by 4
      rf_decim8     a 51-tap RF filter and decimation by 8 (a 1.92 MS/s capture: the multiplex still at
                    240 kS/s): the generic FE inside the receiver, on u8 IQ"""
    kw, lens = CONFIGS[name]
    kw = dict(kw)
    rf_taps = kw.pop("rf_taps", 151)
    _check_case(sdr, gpu_ctx, oracle, lens[big], 1, seed0=210, kw=kw, rf_taps=rf_taps, tag=name)


@gpu
@pytest.mark.parametrize("name", list(DEV_FEEDS))
def test_rx_generic_fe_from_device_rows(sdr, gpu_ctx, oracle, name):
    """B = 16 007 from device memory (sdr_rx_process_dev) where the tiled FE kernels cannot take
    the rows -- an odd f32 row stride with S = 3, an f32 base 8 bytes past a 16-byte boundary, a
    u8 base 2 bytes past a 4-byte boundary (one stream, and two streams B + 3 apart; the receiver
    hands the generic kernels such u8 rows as f32): the generic FE branch against the oracle -- and,
    beside the odd stride, the even stride B + 1 (the tiled kernels on rows with one complex sample
    of foreign data between them)."""
    f = DEV_FEEDS[name]
    B, S = 16_007, f["S"]
    es = np.dtype(f["dtype"]).itemsize
    # (sdr_rx_process_dev, csrc/rx.hip: fast needs an even f32 stride for S > 1 and a base aligned to 16 / 4 bytes)
    generic = (S > 1 and f["dtype"] == np.float32 and (B + f["pad"]) % 2 != 0) or \
        (2 * f["lead"] * es) % (16 if f["dtype"] == np.float32 else 4) != 0
    assert generic == f["generic"]
    _check_case(sdr, gpu_ctx, oracle, B, S, seed0=220, dev_feed=f, tag=name)


# ---- on the CPU ------------------------------------------------------------------------------------
def test_shape_table_geometry():
    """What the shape table says each row is the smallest case of, from the copied constants."""
    geo = {B: (rx_replay.lengths(B), long_geom(rx_replay.lengths(B)[0])) for B, _ in SHAPES}
    assert geo[7][0] == (1, 1, 1)
    assert geo[1_003][0] == (101, 21, 24) and 101 < 150
    assert geo[16_007][0][0] == 1_601 and 16_007 % 10 != 0
    assert geo[163_850][0][0] == SDR_PLL_BLOCK_MAX and geo[163_850][1] == (False, 16_385, 1)
    assert geo[163_880][1] == (True, LONG_PB, 2) and 16_388 - LONG_PB == 2_052 and LONG_PB % TH32_LINE == 0
    assert geo[286_730][1] == (True, 9_558, 3) and 9_558 % TH32_LINE != 0 and not is_span(28_673)
    (M, A, R), _ = geo[327_680]
    assert is_span(M) and M == 32 * MM_WT and M % 5 == 3 and A == 6_554 and R == 7_783 == 6 * CR_TO + 487
    assert is_span(32_772) and 32_772 - 32 * MM_WT == 4 and geo[327_720][0][0] == 32_772
    assert geo[327_700][0][0] == 32_770 and not is_span(32_770) and geo[327_700][1][0]
    assert geo[329_995][0][0] == 33_000 and is_span(33_000) and 33_000 - 32 * MM_WT == 232 and 329_995 % 10 != 0
    for _, lens in CONFIGS.values():
        assert lens[0] in (16_007, 12_807) and lens[1] in (327_720, 262_176)
    assert rx_replay.lengths(12_807, 8)[0] == 1_601 and rx_replay.lengths(262_176, 8)[0] == 32_772


@pytest.mark.parametrize("B", [1_003, 15_360])
def test_replay_reproduces_the_oracle_block_loops(oracle, B):
    """The reference is the reference: fed the oracle's own rows, the per-stage replay gives
    oracle.mono_stereo_blocks and oracle.rds_blocks (model/fmMonoBlock.py:80-173,
    model/fmRDSblock.py:127-204) over a 3-block u8 stream to 1e-12, every row, every block, and
    their carried demod phase."""
    import rtsdr
    nb = 3
    u8 = rtsdr.synth.fm_iq(nb * B + 1, seed=5, dtype=np.uint8)     # (+ 1: the loops' strict "<")
    f = _norm(u8)
    mono = oracle.mono_stereo_blocks(f, B, rf_taps=151, audio_taps=151, nblocks=nb)
    rds = oracle.rds_blocks(u8, 2 * B, taps=151, nblocks=nb)
    assert len(mono) == nb and len(rds) == nb
    replay = rx_replay.Replay(oracle, 1, _taps(oracle), pll_fn=oracle.fm_pll)
    M, want_n = _expect_lengths(B, 10, 5)
    worst = 0.0
    for k in range(nb):
        rows = {nm: [(rds[k] if nm in RDS_TOL else mono[k])[nm]] for nm in ALL}
        ref = replay.block([f[2 * k * B:2 * (k + 1) * B]], rows)
        assert sorted(ref) == sorted(ALL)
        for nm in ALL:
            assert ref[nm][0].shape == rows[nm][0].shape == (want_n[nm],), (nm, k)
            worst = max(worst, maxabs(ref[nm][0], rows[nm][0]))
        assert abs(replay.state()[0][0] - mono[k]["phase"]) <= 1e-12
    assert worst <= 1e-12, worst
