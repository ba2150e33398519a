"""The multi-stream block receiver (sdr_rx_*, csrc/rx.hip; its stage kernels, csrc/rx_stage.hip)
on the GPU: SURVEY §8a C5 --
8 independent u8 streams (seeds 0-7, B = 153 600 complex, src/fm_radio.cpp:23) through
mono + stereo + RDS to the RRC output at once -- against the CPU oracle's restatement of
model/fmMonoBlock.py:80-173 and model/fmRDSblock.py:127-204, with every state carried across
blocks on the device.

Tolerances (f32 kernels vs the f64 oracle):
  audio / stereo / L / R     RMS <= 1e-6, max <= 1e-5        (north_star: 1e-6 RMS)
  demod                      RMS <= 1e-6, max <= 1e-5
  RDS chain, relative to each signal's peak: see RDS_TOL (measured on MI355X, bound ~3x)
"""
import numpy as np
import pytest

from conftest import long_blocks, maxabs, rms

pytestmark = pytest.mark.gpu

B5 = 153_600
AUDIO_RMS, AUDIO_MAX = 1e-6, 1e-5
# stereo NCO (f32 cos of the f64 phase) vs the oracle: 3e-8 is the f32 rounding; ~3x margin
# over the worst measured on MI355X (tests/test_dropin.py bounds the same quantity at 1e-7)
NCO_MAX = 1e-7

# (max, rms) relative to max|ref| per RDS intermediate: about 3x the worst errors measured on
# MI355X over 8 streams x 2 blocks (profiles/r02/rx_tolerances.log).  The Q branch is small
# next to its own peak (the carrier is locked onto I), so its relative error is larger.
RDS_TOL = {
    "extract": (4e-6, 8e-7), "pre_pll": (5e-6, 1e-6), "nco_i": (1e-7, 5e-8), "nco_q": (1e-7, 5e-8),
    "lpf_i": (5e-6, 1e-6), "lpf_q": (3e-5, 8e-6), "resample_i": (3e-6, 8e-7), "resample_q": (3e-5, 8e-6),
    "rrc_i": (4e-6, 8e-7), "rrc_q": (3e-5, 7e-6),
}


def _streams(sdr, S, nblocks, seed0=0):
    # one extra complex sample: the reference loops run while (k+1)*B < len (strict)
    return np.stack([sdr.synth.fm_iq(nblocks * B5 + 1, seed=seed0 + s, dtype=np.uint8) for s in range(S)])


def test_receiver_c5_eight_streams_match_oracle(sdr, gpu_ctx, oracle):
    """C5: 8 streams x 2 blocks, mono + stereo + RDS, one receiver; every stream's outputs
    against the oracle's per-stream block loops (u8 normalised as fmRDSblock.py:58-59)."""
    S, nb = 8, 2
    iq = _streams(sdr, S, nb)
    rx = sdr.Receiver(S, B5, stereo=True, rds=True, iq_dtype=np.uint8)
    names = ["demod", "audio", "stereo", "left", "right", "bpf_recovery", "nco", "bpf_extraction"] + list(RDS_TOL)
    got = []
    gpu_ctx.pll_stats(reset=True)
    for k in range(nb):
        got.append(rx.process(iq[:, 2 * k * B5:2 * (k + 1) * B5], fetch=names))
        if k == 0:
            first = rx.pll_stats(reset=True)
    st = rx.pll_stats()
    print("solver counters, block 0:", first, "block 1:", st)
    npb = long_blocks(B5 // 10)                      # pseudo-blocks per block and PLL
    assert first["recurrences"] == 2 * S * npb and st["recurrences"] == 2 * S * npb
    # after the acquisition block every stereo and RDS recurrence completes in the parallel solve
    assert st["spec_r0"] + st["spec_r1"] + st["spec_r2"] == 2 * S * npb and st["sequential"] == 0, st
    worst = {}
    nco_worst = 0.0
    for s in range(S):
        f = (iq[s].astype(np.float64) - 128.0) / 128.0
        mono = oracle.mono_stereo_blocks(f, B5, rf_taps=151, audio_taps=151, nblocks=nb)
        rds = oracle.rds_blocks(iq[s], 2 * B5, taps=151, nblocks=nb)
        for k in range(nb):
            g = got[k]
            assert rms(g["demod"][s], mono[k]["demod"]) < 1e-6, (s, k)
            for key in ("audio", "stereo", "left", "right"):
                assert rms(g[key][s], mono[k][key]) < AUDIO_RMS, (key, s, k, rms(g[key][s], mono[k][key]))
                assert maxabs(g[key][s], mono[k][key]) < AUDIO_MAX, (key, s, k)
            nco_worst = max(nco_worst, maxabs(g["nco"][s], mono[k]["nco"]))
            assert maxabs(g["nco"][s], mono[k]["nco"]) < NCO_MAX, (s, k)
            for key, (tmax, trms) in RDS_TOL.items():
                ref = rds[k][key]
                scale = max(float(np.max(np.abs(ref))), 1e-3)
                em, er = maxabs(g[key][s], ref) / scale, rms(g[key][s], ref) / scale
                worst[key] = max(worst.get(key, (0, 0))[0], em), max(worst.get(key, (0, 0))[1], er)
                assert em < tmax and er < trms, (key, s, k, em, er)
    print("RDS relative errors (max, rms):", {k: (f"{a:.1e}", f"{b:.1e}") for k, (a, b) in worst.items()},
          f"stereo NCO max error {nco_worst:.1e}")


def test_receiver_streams_equal_single_stream(sdr, gpu_ctx):
    """Batching is exact: stream s of a 3-stream receiver == a 1-stream receiver on s (same
    kernels, same per-stream tiling), for every output, across 3 blocks (f32 IQ, 51 200)."""
    B = 51_200
    S, nb = 3, 3
    iq = np.stack([sdr.synth.fm_iq(nb * B, seed=30 + s) for s in range(S)])
    kw = dict(stereo=True, rds=True, iq_dtype=np.float32)
    multi = sdr.Receiver(S, B, **kw)
    singles = [sdr.Receiver(1, B, **kw) for _ in range(S)]
    for k in range(nb):
        blk = iq[:, 2 * k * B:2 * (k + 1) * B]
        mo = multi.process(blk, fetch=multi.outputs)
        for s in range(S):
            so = singles[s].process(blk[s], fetch=multi.outputs)
            for name in multi.outputs:
                assert np.array_equal(mo[name][s], so[name][0]), (name, s, k)
    ph_m, ps_m, pr_m = multi.state()
    for s in range(S):
        ph, ps, pr = singles[s].state()
        assert ph_m[s] == ph[0] and np.array_equal(ps_m[s], ps[0]) and np.array_equal(pr_m[s], pr[0])


def test_receiver_carried_state_matches_oracle(sdr, gpu_ctx, oracle):
    """Two f32 streams, 4 blocks of the reference's 51 200 (fmMonoBlock.py:53): the demod
    phase and the stereo PLL state after each block == the oracle's carried values."""
    B, S, nb = 51_200, 2, 4
    iq = np.stack([sdr.synth.fm_iq(nb * B + 1, seed=50 + s) for s in range(S)])
    rx = sdr.Receiver(S, B, stereo=True, iq_dtype=np.float32)
    ref = [oracle.mono_stereo_blocks(iq[s], B, rf_taps=151, audio_taps=151, nblocks=nb) for s in range(S)]
    st_ref = [[0.0, 0.0, 1.0, 0.0, 1.0, 0.0] for _ in range(S)]
    for k in range(nb):
        o = rx.process(iq[:, 2 * k * B:2 * (k + 1) * B], fetch=["audio", "left", "right", "nco"])
        ph, ps, _ = rx.state()
        for s in range(S):
            r = ref[s][k]
            assert abs(ph[s] - r["phase"]) < 1e-5, (s, k)
            _, _, st_ref[s] = oracle.fm_pll(r["bpf_recovery"], 19e3, 240e3, list(st_ref[s]), 2)
            assert maxabs(ps[s], st_ref[s]) < 1e-5, (s, k, ps[s], st_ref[s])
            for key in ("audio", "left", "right"):
                assert rms(o[key][s], r[key]) < AUDIO_RMS, (key, s, k)


def test_receiver_reset_restarts_the_stream(sdr, gpu_ctx):
    B = 51_200
    iq = sdr.synth.fm_iq(2 * B, seed=3)
    rx = sdr.Receiver(1, B, stereo=True, iq_dtype=np.float32)
    a0 = rx.process(iq[:2 * B])["left"]
    rx.process(iq[2 * B:])
    rx.reset()
    assert np.array_equal(rx.process(iq[:2 * B])["left"], a0)


def test_receiver_argument_errors(sdr, gpu_ctx):
    import ctypes
    from importlib import import_module
    _lib = import_module("real-time-software-defined-radio_amd._lib")
    rx = sdr.Receiver(2, 1000, iq_dtype=np.float32)
    with pytest.raises(ValueError):
        rx.process(np.zeros(2 * 1000, np.float32))                  # one stream's worth for two
    rx.process(np.zeros((2, 2000), np.float32))
    with pytest.raises(ValueError):                                   # taps after the first block
        b = np.ones(5)
        _lib.check(rx.lib.sdr_rx_set_filter(rx.handle, 0, _lib.f64p(b), 5), "set_filter")
    with pytest.raises(ValueError):
        rx.output("rrc_i")                                            # not produced without RDS
    h = ctypes.c_void_p()
    _lib.check(gpu_ctx.lib.sdr_rx_create(gpu_ctx.handle, 1, 100, 0, 0, ctypes.byref(h)), "create")
    with pytest.raises(ValueError, match="taps are not set"):
        _lib.check(gpu_ctx.lib.sdr_rx_process(h, np.zeros(200, np.float32).ctypes.data, 100), "process")
    gpu_ctx.lib.sdr_rx_destroy(h)
    with pytest.raises(ValueError):
        _lib.check(gpu_ctx.lib.sdr_rx_create(gpu_ctx.handle, 1, 100, 0, 8, ctypes.byref(h)), "bad flags")


@pytest.mark.parametrize("pipeline,depth,fetch", [(False, 1, "all"), (True, 1, "all"), (False, 2, "all"),
                                                  (True, 2, "all"), (True, 3, "all"), (True, 1, "stage"),
                                                  (True, 2, "stage"), (True, 3, "stage")])
def test_receiver_submit_equals_process(sdr, gpu_ctx, pipeline, depth, fetch):
    """sdr_rx_submit / sdr_rx_flush (block k launched, block k-depth delivered; r04b: depth 2
    and 3 keep that many blocks in flight, a pipelined receiver then three row sets) ==
    sdr_rx_run block by block, bit for bit -- with and without the two-stream pipeline.
    fetch "all": every output, the stage-stored ones (pinned host stores) and the copied ones
    (demod, NCOs); "stage": only the outputs stage kernels store (the default fetch, the shape
    bench c3 / c4 time), where nothing follows the back half on the stream and the row-set
    event doubles as the block's completion event (csrc/rx.hip sdr_rx_submit)."""
    B, S, nb = 51_200, 2, 6
    iq = np.stack([sdr.synth.fm_iq(nb * B, seed=60 + s) for s in range(S)])
    kw = dict(stereo=True, rds=True, iq_dtype=np.float32)
    ref_rx = sdr.Receiver(S, B, **kw)
    rx = sdr.Receiver(S, B, pipeline=pipeline, depth=depth, **kw)
    names = ref_rx.outputs if fetch == "all" else None
    want = [ref_rx.process(iq[:, 2 * k * B:2 * (k + 1) * B], fetch=names) for k in range(nb)]
    if fetch != "all":
        assert sorted(want[0]) == sorted(["audio", "left", "right", "rrc_i", "rrc_q"])
    got = []
    for k in range(nb):
        prev = rx.submit(iq[:, 2 * k * B:2 * (k + 1) * B], fetch=names)
        assert (prev is None) == (k < depth)
        if prev is not None:
            got.append(prev)
    got.extend(rx.flush())
    assert len(got) == nb
    assert rx.flush() == []
    for k in range(nb):
        assert sorted(got[k]) == sorted(want[k])
        for name in want[k]:
            assert np.array_equal(got[k][name], want[k][name]), (name, k)
    # state after the last block, and a synchronous call after submits
    for a, b in zip(rx.state(), ref_rx.state()):
        assert np.array_equal(a, b)
    rx.reset()
    assert np.array_equal(rx.process(iq[:, :2 * B], fetch=["left"])["left"], want[0]["left"])


@pytest.mark.parametrize("u8,rf_taps", [(True, 151), (False, 101), (False, 51)])
def test_receiver_pipelined_process_dev(sdr, gpu_ctx, u8, rf_taps):
    """Device-resident blocks through a pipelined receiver (front half of block k on its own
    stream beside the back half of block k-1, row sets alternating): == the unpipelined
    receiver, bit for bit, for every output of every block (51 taps: the generic FE path,
    whose front half runs on the context stream)."""
    from importlib import import_module
    _lib = import_module("real-time-software-defined-radio_amd._lib")
    S, nb = 3, 4
    B = 15_360
    dt = np.uint8 if u8 else np.float32
    iq = np.stack([sdr.synth.fm_iq(nb * B, seed=80 + s, dtype=dt) for s in range(S)])
    blocks = np.ascontiguousarray(np.stack([iq[:, 2 * k * B:2 * (k + 1) * B] for k in range(nb)]))
    rf_b, au_b = sdr.design.mono_coeffs(rf_taps, 151)
    kw = dict(stereo=True, rds=True, iq_dtype=dt, rf_coeff=rf_b, audio_coeff=au_b)
    ref_rx = sdr.Receiver(S, B, **kw)
    rx = sdr.Receiver(S, B, pipeline=True, **kw)
    d = _lib.DeviceBuffer.from_array(gpu_ctx, blocks)
    gpu_ctx.synchronize()
    step = blocks[0].nbytes
    names = ref_rx.outputs
    for k in range(nb):
        want = ref_rx.process(blocks[k], fetch=names)
        rx.process_dev(d.ptr + k * step, B)
        if k % 2 == 1:                     # two blocks in flight before the first read
            continue
        for name in names:
            assert np.array_equal(rx.output(name), want[name]), (name, k)
    gpu_ctx.synchronize()
    for name in names:
        assert np.array_equal(rx.output(name), want[name]), (name, "last")
    for a, b in zip(rx.state(), ref_rx.state()):
        assert np.array_equal(a, b)


def test_receiver_set_pll_between_blocks(sdr, gpu_ctx, oracle):
    """sdr_rx_set_pll after the first block (the one setter that stays legal): block 2's stereo
    NCO == the oracle's fmPll on the device's own pilot row, from block 1's carried state, with
    the NEW bandwidth -- the loop's tables follow the current configuration.  Per-block stereo
    receiver, one stream; the per-block tolerance of tests/test_pll_spec.py."""
    from importlib import import_module
    from test_pll_spec import NCO_TOL
    _lib = import_module("real-time-software-defined-radio_amd._lib")
    B, bw = 51_200, 0.02
    iq = sdr.synth.fm_iq(2 * B, seed=90)
    rx = sdr.Receiver(1, B, stereo=True, iq_dtype=np.float32)
    rx.process(iq[:2 * B], fetch=["nco"])
    carried = [float(v) for v in rx.state()[1][0]]
    _lib.check(rx.lib.sdr_rx_set_pll(rx.handle, 0, 19e3, 240e3, 2.0, 0.0, bw), "sdr_rx_set_pll")
    got = rx.process(iq[2 * B:], fetch=["bpf_recovery", "nco"])
    pilot = got["bpf_recovery"][0].astype(np.float64)
    want, _, st_want = oracle.fm_pll(pilot, 19e3, 240e3, list(carried), 2.0, 0.0, bw)
    stale, _, _ = oracle.fm_pll(pilot, 19e3, 240e3, list(carried), 2.0, 0.0, 0.01)
    err, off = maxabs(got["nco"][0], want), maxabs(got["nco"][0], stale)
    print(f"stereo NCO after set_pll: max error {err:.2e} vs the new loop, {off:.2e} vs the old one")
    assert err < NCO_TOL
    assert off > NCO_TOL                       # (the input tells the two loops apart)
    assert maxabs(rx.state()[1][0], st_want) < 1e-6


@pytest.mark.parametrize("de", [None, 75e-6])
def test_receiver_outputs_match_the_library(sdr, gpu_ctx, de):
    """Receiver.outputs (blocks.py's _produces, answered before the library object is finalised) names
    exactly the outputs sdr_rx_output accepts (kOutput, csrc/rx_layout.h), for every flag combination,
    with de-emphasis wherever the flags produce audio.  The smallest block; no IQ is processed."""
    from importlib import import_module
    names = import_module("real-time-software-defined-radio_amd._lib").RX_OUTPUTS
    for mono in (False, True):
        for stereo in (False, True):
            for rds in (False, True):
                rx = sdr.Receiver(1, 1, mono=mono, stereo=stereo, rds=rds, deemphasis=de if mono or stereo else None)
                try:
                    accepted = []
                    for name in names:
                        try:
                            rx.output_ptr(name)
                            accepted.append(name)
                        except ValueError as e:            # only the library's "not produced" answer counts
                            assert "is not produced by flags" in str(e), (name, str(e))
                    assert rx.outputs == accepted, (mono, stereo, rds, de)
                finally:
                    rx.close()
