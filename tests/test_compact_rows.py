"""The compact phase rows (csrc/sdr_nco.h "compact phase rows") on the CPU: the
pilot loop's phaseEst (model/fmPll.py:22-37, restated per step) on the oracle's pilot-BPF rows
of a synthetic FM stream, cut into 32-row lines, and the angle error the f32 residual's
rounding makes (x ncoScale 2, model/fmMonoBlock.py:119):

  * sloped lines (start + slope over the line, as the solve sets them from its previous pass
    over a chunk -- here the exact trajectory, what a round-0 solve's guess follows): the bound
    the NCO replay tolerance of tests/test_span.py counts on, at acquisition and once locked;
  * flat lines at a chunk's start (the solve's AF check form, middle pseudo-blocks only, i.e.
    after the first 14 336 steps of a stream): locked-loop rounding;
  * the acquisition is why the first pseudo-block keeps the slopes: a flat line there rounds
    ~5x worse.

The same three forms -- and seq_run's ({phase, integrator} at a line's first row) -- on the
adverse inputs of tests/adverse_input.py (both loops), whose lock state is checked here too:
the bounds tests/test_span_adverse.py relies on.

And the matrix-core mixers' folded angle (sdr_nco.h nco4_eval_w<TH32>) against the direct
form, in f64 on the host: the same angle to rounding."""
import math

import numpy as np
import pytest

B5 = 153_600
LINE = 32
PB = 14_336           # pll.hip LONG_PB: the first pseudo-block of a stream


def _loop(x, freq, bw):
    """fmPll's phaseEst and integrator after every step (model/fmPll.py:22-37, restated per step)
    on the loop input x, from the stream-start state"""
    kp, ki = bw * 2.666, bw * bw * 3.555              # model/fmPll.py:4-10
    w = 2 * math.pi * freq / 240e3
    integ = phase = 0.0
    fi, fq = 1.0, 0.0
    ph, it = np.empty(len(x)), np.empty(len(x))
    for k in range(len(x)):
        e = math.atan2(x[k] * (-fq), x[k] * fi)
        integ += ki * e
        phase += kp * e + integ
        arg = w * (k + 1) + phase
        fi, fq = math.cos(arg), math.sin(arg)
        ph[k] = phase
        it[k] = integ
    n = len(ph) // LINE * LINE
    return ph[:n].reshape(-1, LINE), it[:n].reshape(-1, LINE)


LOOPS = {"pilot": ("bpf_recovery", 19e3, 0.01, 2.0), "rds": ("pre_pll", 114e3, 0.001, 0.5)}   # input, Hz, bandwidth, ncoScale
SPANS = {"clean": 1, "J": 1, "S": 1, "U": 1, "D": 2}   # K = 3 spans modelled per input
ADVERSE = ("J", "S", "U", "D")


@pytest.fixture(scope="module")
def loop_phases(oracle):
    """input name -> {"pilot" / "rds": (phaseEst, integrator), each as lines of 32 rows}: both
    loops of the receiver on the oracle's loop inputs -- "clean" is synth.fm_iq seed 0, the others
    tests/adverse_input.py's cases (seed 5), over SPANS[name] spans of 3 blocks"""
    import rtsdr
    from adverse_input import CASES, adverse_iq
    cache = {}

    def get(name):
        if name not in cache:
            nblk = 3 * SPANS[name]
            if name == "clean":
                f = rtsdr.synth.fm_iq(nblk * B5 + 1, seed=0)
            else:
                u8 = adverse_iq(nblk * B5 + 1, 5, **CASES[name])
                f = (u8.astype(np.float64) - 128.0) / 128.0
            mono = oracle.mono_stereo_blocks(f, B5, nblocks=nblk, pll_fn=oracle.fm_pll_c)
            rows = {"bpf_recovery": np.concatenate([b["bpf_recovery"] for b in mono])}
            if name != "clean":
                rds = oracle.rds_blocks(u8, 2 * B5, nblocks=nblk, pll_fn=oracle.fm_pll_c)
                rows["pre_pll"] = np.concatenate([b["pre_pll"] for b in rds])
            cache[name] = {lp: _loop(rows[src], hz, bw) for lp, (src, hz, bw, _) in LOOPS.items() if src in rows}
        return cache[name]
    return get


@pytest.fixture(scope="module")
def pilot_phases(loop_phases):
    return loop_phases("clean")["pilot"][0]


def _angle_err(r, scale=2.0):
    return np.abs(r.astype(np.float32).astype(np.float64) - r) * scale     # x ncoScale


def _prev(P):
    return np.concatenate([[0.0], P[:-1, -1]])        # the phase before each line's first row


def _sloped(P):
    """residuals against the line through a 32-step segment's start and end (the solve's form)"""
    prev = _prev(P)
    s = (P[:, -1] - prev) / LINE
    return P - ((prev + s)[:, None] + s[:, None] * np.arange(LINE))


def _flat(P):
    """residuals against the phase before the line's first row (the solve's AF check form)"""
    return P - _prev(P)[:, None]


def _seq(P, I):
    """residuals against {phase, integrator} at the line's first row (pll.hip seq_run's form)"""
    return P - (P[:, :1] + I[:, :1] * np.arange(LINE))


def model_errors(loop_phases, name):
    """the three line forms' worst angle error (f32 residual rounding x ncoScale) on an input, over
    both loops: {"sloped", "seq", "flat_mid" (the flat form past the first pseudo-block)}"""
    out = {"sloped": 0.0, "seq": 0.0, "flat_mid": 0.0}
    for lp, (P, I) in loop_phases(name).items():
        scale = LOOPS[lp][3]
        out["sloped"] = max(out["sloped"], float(_angle_err(_sloped(P), scale).max()))
        out["seq"] = max(out["seq"], float(_angle_err(_seq(P, I), scale).max()))
        out["flat_mid"] = max(out["flat_mid"], float(_angle_err(_flat(P), scale)[PB // LINE:].max()))
    return out


def test_sloped_lines_round_below_the_replay_tolerance(pilot_phases):
    P = pilot_phases
    prev = np.concatenate([[0.0], P[:-1, -1]])        # the phase before each line's first row
    s = (P[:, -1] - prev) / LINE
    a = prev + s
    r = P - (a[:, None] + s[:, None] * np.arange(LINE))
    e = _angle_err(r)
    print(f"sloped lines: max angle error {e.max():.2e} rad (after 2 000 steps {e[2000 // LINE:].max():.2e}), "
          f"max |r| {np.abs(r).max():.3f} rad")
    assert e.max() < 4e-8                              # measured 2.3e-8 (acquisition)
    assert e[2000 // LINE:].max() < 1.5e-8             # measured 7.5e-9 (locked)


def test_flat_lines_after_the_first_pseudo_block(pilot_phases):
    P = pilot_phases
    prev = np.concatenate([[0.0], P[:-1, -1]])
    r = P - prev[:, None]
    e = _angle_err(r)
    af = e[PB // LINE:]
    print(f"flat lines: max angle error {af.max():.2e} rad past step {PB}, {e.max():.2e} over the stream, "
          f"max |r| past step {PB} {np.abs(r[PB // LINE:]).max():.3f} rad")
    assert af.max() < 3e-8                             # measured 1.5e-8
    assert e.max() > 4e-8                              # at acquisition a flat line would not do (1.1e-7)


def _wander(P, offset_hz, win=2048):
    """the pilot loop's phase less the carrier's drift, peak to peak per window of `win` steps"""
    ph = P.reshape(-1)
    ph = ph - 2 * math.pi * offset_hz / 240e3 * np.arange(1, len(ph) + 1)
    w = ph[:len(ph) // win * win].reshape(-1, win)
    return w.max(axis=1) - w.min(axis=1)


def test_adverse_inputs_stay_adverse(loop_phases):
    """tests/adverse_input.py's cases do to the pilot loop what tests/test_span_adverse.py needs
    of them: J locked but jittery, S slipping cycles, U never locked, D locked except around each
    pilot gap (one per K = 3 span, inside the span's second pseudo-block) where it wanders by
    whole turns and re-locks"""
    from adverse_input import CASES
    tau = 2 * math.pi
    w = {c: _wander(loop_phases(c)["pilot"][0], CASES[c].get("pilot_offset_hz", 0.0)) for c in ADVERSE}
    for c in ADVERSE:
        print(f"{c}: pilot phase wander per 2 048 steps (rad):", np.array2string(w[c], precision=1, floatmode="fixed"))
    assert np.all(w["J"][1:] < tau)
    assert np.sum(w["S"] > tau) >= 3
    assert np.sum(w["U"] > tau) >= len(w["U"]) / 2
    # (windows count from the stream start; one belongs to a range when it overlaps it.  Window 0
    # is the acquisition from phase 0, as on the clean capture: ~pi on any input)
    start = np.arange(len(w["D"])) * 2048
    outside = start > 0
    for lo, hi in ((16_384, 22_528), (62_464, 68_608)):
        inside = (start + 2048 > lo) & (start < hi)
        assert np.any(w["D"][inside] > tau), (lo, hi)
        assert PB <= lo % (3 * B5 // 10) and hi % (3 * B5 // 10) <= 2 * PB      # a middle pseudo-block of its span
        outside &= ~inside
    assert np.all(w["D"][outside] < 0.5)


# what the NCO replay check of tests/test_span_adverse.py can always count on is 6e-8 (the f32
# rounding of the NCO value) + the worst of these two forms over the adverse inputs, and that must
# stay <= 2.0e-7 (the device measures below tests/test_span.py's NCO_REPLAY, which the check uses)
SLOPED_MAX = 4e-8
SEQ_MAX = 1.2e-7


def test_line_forms_on_adverse_inputs(loop_phases):
    """What each line form of the compact rows costs on unlocked and re-acquiring loops (both
    loops, f32 residual rounding x ncoScale): the sloped form keeps the locked-loop bound, seq_run's
    form ({phase, integrator} at the line's first row) is computed -- E_seq -- and bounded by
    SEQ_MAX, and a flat line in a middle pseudo-block exceeds the whole replay tolerance of
    tests/test_span.py (1.5e-7) wherever the loop is not locked there: why the solve may take the
    flat form only where the loop hardly moves"""
    E = {c: model_errors(loop_phases, c) for c in ADVERSE}
    for c in ADVERSE:
        print(f"{c}: " + ", ".join(f"{k} {v:.2e}" for k, v in E[c].items()))
    for c in ADVERSE:
        assert E[c]["sloped"] < SLOPED_MAX, (c, E[c])
        assert E[c]["seq"] < SEQ_MAX, (c, E[c])
    for c in ("S", "U", "D"):
        assert E[c]["flat_mid"] > 1.5e-7, (c, E[c])
    assert 6e-8 + max(SLOPED_MAX, SEQ_MAX) <= 2.0e-7


def test_folded_mixer_angle_equals_the_direct_form():
    rng = np.random.default_rng(7)
    ws = 2 * math.pi * 19e3 / 240e3 * 2.0             # w scale
    scale = 2.0
    worst = 0.0
    for _ in range(2000):
        base = rng.uniform(-math.pi, math.pi)
        a = rng.uniform(-50.0, 50.0)
        s = rng.uniform(-1e-3, 1e-3)
        o = int(rng.integers(0, 29)) & ~3            # a group's first row within its line
        dk = int(rng.integers(-4, 1500))             # output index relative to the window's reference
        r = rng.uniform(-0.3, 0.3, 4).astype(np.float32).astype(np.float64)
        w2 = scale * s + ws
        g = scale * (s * (o - dk) + a) + base
        for e in range(4):
            folded = r[e] * scale + (w2 * (dk + e) + g)
            direct = (a + s * (o + e) + r[e]) * scale + (ws * (dk + e) + base)
            worst = max(worst, abs(folded - direct))
    print(f"folded vs direct angle: {worst:.2e} rad")
    assert worst < 1e-11
