"""The symbol-clock specification (rtsdr.RdsSymbolClock, rdsclock.py) on synthetic rows, CPU only.

Rows come from tests/rds_clock_rows.py: 40 coded groups (160 blocks), raised-cosine pulses at
24 (1 + ppm 1e-6) samples a symbol, white noise sigma.  The measure is the number of the generator's
blocks that RdsBlockSync reports with status <= 1.  Counts on these rows (seed 3; new path / the
existing rule = oracle.rds_link on the whole row as one block):

    +500 ppm sigma 0.3   158 / 66        -500 ppm sigma 0.3   158 / 61
    +1000 ppm sigma 0.3  158 / 57        -1000 ppm sigma 0.3  158 / 57
    -500 ppm sigma 0.5   158 / 42        0 ppm sigma 0.05     159 / 159
    delays 0 .. 23 at 0 ppm, sigma 0.05 (seed 4): 158 or 159

The bounds below are the issue's: the new path keeps at least 150 of 160 where the existing rule
loses at least a third (at most 106), and at least 157 over the delays.
"""
import numpy as np
import pytest

import rds_clock_rows as rc

DRIFT = [(500, 0.3), (-500, 0.3), (1000, 0.3), (-1000, 0.3), (-500, 0.5)]


@pytest.mark.parametrize("delay", range(24))
def test_delays(sdr, delay):
    got = rc.clock_blocks(sdr, rc.row(delay=delay, seed=4), 4)
    print("delay", delay, "blocks", got)
    assert got >= 157


@pytest.mark.parametrize("ppm,sigma", DRIFT)
def test_drift_beside_the_existing_rule(sdr, oracle, ppm, sigma):
    x = rc.row(ppm=ppm, sigma=sigma, seed=3)
    new, old = rc.clock_blocks(sdr, x, 3), rc.link_blocks(sdr, oracle, x, 3)
    print("ppm", ppm, "sigma", sigma, "clock", new, "existing rule", old)
    assert new >= 150
    assert old <= 160 * 2 // 3


def test_no_drift_loses_nothing(sdr, oracle):
    """at 0 ppm the tracker is as good as the fixed offset"""
    x = rc.row(seed=3)
    assert rc.clock_blocks(sdr, x, 3) >= rc.link_blocks(sdr, oracle, x, 3) >= 157


def _same(sdr, x, cuts, **kw):
    one = rc.model_calls(sdr, x, [len(x)], **kw)[0]
    calls = rc.model_calls(sdr, x, cuts, **kw)
    np.testing.assert_array_equal(np.concatenate([c[0] for c in calls]), one[0])
    assert calls[-1][1] == one[1]
    return one


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_cuts(sdr, seed):
    x = rc.row(ppm=(-1000, 700, 1000)[seed - 1], sigma=0.3, seed=3)
    cuts = rc.random_cuts(len(x), seed)
    assert 0 in cuts and any(0 < c < 768 for c in cuts) and max(cuts) > 2 * 768
    one = _same(sdr, x, cuts)
    assert one[1][8] > 0                                           # the row wraps phi


@pytest.mark.parametrize("size", [1, 23, 767, 768, 769])
@pytest.mark.parametrize("window", [1, 4])
def test_equal_cuts(sdr, size, window):
    x = rc.row(ppm=1000, delay=20, sigma=0.3, seed=5, groups=6)   # about 30 k samples
    cuts = [size] * (len(x) // size) + ([len(x) % size] if len(x) % size else [])
    one = _same(sdr, x, cuts, window=window)
    assert one[1][8] > 0 and one[1][1] == len(x) // 768


@pytest.mark.parametrize("ppm", [1000, -1000, 500, -500])
def test_wraps(sdr, ppm):
    """phi goes round: the instants stay 23 .. 25 apart, no symbol is dropped or repeated"""
    x = rc.row(ppm=ppm, sigma=0.3, seed=3)
    clk = sdr.RdsSymbolClock()
    clk.process(x)
    consumed, segments, phi, pi, symbols, bits, fwd, back, wraps, changes = clk.state()
    inst = np.array(clk.instants)
    assert len(inst) == symbols and set(np.diff(inst).tolist()) <= {23, 24, 25}
    assert {24, 25 if ppm > 0 else 23} <= set(np.diff(inst).tolist())
    assert wraps >= 3 and (fwd if ppm > 0 else back) >= 90 and changes == 0
    assert consumed == 768 * segments == len(x) // 768 * 768
    # 32 a segment, one fewer for a wrap forward and one more for a wrap back
    assert symbols == 32 * segments - (wraps if ppm > 0 else -wraps)
    # ... which is what the transmitter sent in the consumed samples
    assert abs(symbols - consumed / (24 * (1 + ppm * 1e-6))) <= 1.0
    assert 0 <= inst[0] < 24 and consumed - 25 <= inst[-1] < consumed
    np.testing.assert_array_equal(np.array(clk.symbol_values, dtype=np.float32), x[inst])


def test_wraps_both_ways_in_one_row(sdr):
    x = np.concatenate([rc.row(ppm=1000, sigma=0.3, seed=3), rc.row(ppm=-1000, sigma=0.3, seed=6)])
    clk = sdr.RdsSymbolClock()
    inst = []
    for o in range(0, len(x), 50_000):
        clk.process(x[o:o + 50_000])
        inst += clk.instants
    st = clk.state()
    assert st[6] >= 150 and st[7] >= 150 and st[8] >= 10
    assert set(np.diff(inst).tolist()) == {23, 24, 25} and len(inst) == st[4]


@pytest.mark.parametrize("insert_at", [4001, 4002])
def test_inserted_symbol(sdr, insert_at):
    """one extra symbol: the pairing moves once, within window + 1 segments"""
    x = rc.row(seed=3, insert_at=insert_at)
    clk = sdr.RdsSymbolClock()
    seg_of_insert = (12 + 24 * insert_at) // 768
    moved = []
    for g in range(len(x) // 768):
        before = clk.state()[3]
        clk.process(x[768 * g:768 * (g + 1)])
        if clk.state()[3] != before:
            moved.append(g)
    assert len(moved) == 1 and clk.state()[9] == 1
    assert seg_of_insert <= moved[0] <= seg_of_insert + clk.window + 1
    # without one, never
    plain = sdr.RdsSymbolClock()
    plain.process(rc.row(seed=3))
    assert plain.state()[9] == 0


def test_first_pairing_is_either_parity(sdr):
    """a row that starts one symbol late pairs on the other parity and gives the same blocks"""
    x = rc.row(seed=3)
    a, b = sdr.RdsSymbolClock(), sdr.RdsSymbolClock()
    da, db = a.process(x), b.process(x[24:])
    assert {a.state()[3], b.state()[3]} == {0, 1}
    assert rc.generator_blocks(sdr.RdsBlockSync().process(db), 3) >= 157 <= rc.generator_blocks(sdr.RdsBlockSync().process(da), 3)


@pytest.mark.parametrize("window", [1, 4, 16])
def test_warm_up(sdr, window):
    """phi over the first segments against sums written out here: segment g < window sees g + 1"""
    x = rc.row(ppm=300, delay=7, sigma=0.5, seed=8, groups=6)
    clk = sdr.RdsSymbolClock(window=window)
    E, phi = [], None
    for g in range(20):
        seg = x[768 * g:768 * (g + 1)].astype(np.float64)
        e = [0.0] * 24
        for j in range(32):
            for p in range(24):
                e[p] += seg[24 * j + p] * seg[24 * j + p]
        E.append(e)
        A = [0.0] * 24
        for w in range(max(0, g - window + 1), g + 1):
            A = [a + b for a, b in zip(A, E[w])]
        phat = A.index(max(A))
        if phi is None:
            phi = phat
        else:
            d = ((phat - phi + 12) % 24) - 12
            phi = (phi + (d >= 2) - (d <= -2)) % 24
        clk.process(x[768 * g:768 * (g + 1)])
        assert clk.state()[1:3] == (g + 1, phi), g


def test_non_finite_samples(sdr):
    """A non-finite sample counts as 0 in the energy and is sampled as it is: NaN and -inf compare
    as 'not above', like 0, so the state is that of the row with zeros in their places."""
    x = rc.row(ppm=200, sigma=0.3, seed=9, groups=6).copy()
    at = np.random.default_rng(1).choice(len(x), 300, replace=False)
    bad, zeroed = x.copy(), x.copy()
    bad[at[0::2]], bad[at[1::2]], zeroed[at] = np.nan, -np.inf, 0.0
    a, b = sdr.RdsSymbolClock(), sdr.RdsSymbolClock()
    da, db = a.process(bad), b.process(zeroed)
    assert a.state() == b.state() and a.instants == b.instants and len(da) == len(db)
    hit = np.isin(a.instants, at)
    assert hit.sum() >= 5 and not np.isfinite(np.array(a.symbol_values)[hit]).any()
    # +inf is above everything: the energy still ignores it
    up = x.copy()
    up[at] = np.inf
    c = sdr.RdsSymbolClock()
    c.process(up)
    assert c.state()[:3] == b.state()[:3] and c.state()[6:9] == b.state()[6:9]
    # a row of nothing but NaN keeps a defined state
    d = sdr.RdsSymbolClock()
    out = d.process(np.full(768 * 5 + 3, np.nan, dtype=np.float32))
    assert d.state() == (3840, 5, 0, 0, 160, 80, 0, 0, 0, 0) and not out.any() and len(out) == 79


def test_short_and_empty_calls(sdr):
    clk = sdr.RdsSymbolClock()
    assert len(clk.process(np.zeros(0, dtype=np.float32))) == 0 and clk.state() == (0,) * 10
    assert len(clk.process(rc.row(seed=3)[:767])) == 0 and clk.state() == (0,) * 10
    d = clk.process(rc.row(seed=3)[767:768])                      # 32 symbols: 16 pairs on parity 0, 15 on 1
    assert clk.state()[:2] == (768, 1) and len(d) == clk.state()[5] - 1 == 15 - clk.state()[3]
    clk.reset()
    assert clk.state() == (0,) * 10


def test_parameters(sdr):
    for kw in (dict(window=0), dict(window=17), dict(hysteresis=-1)):
        with pytest.raises(ValueError):
            sdr.RdsSymbolClock(**kw)
