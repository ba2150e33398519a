"""Device-side RDS symbol clock (RdsClockBank, csrc/rds_clock.hip) against the host model.

rtsdr.RdsSymbolClock is the specification (tests/test_rds_clock_model.py pins it on the CPU): every
expected bit, count and state here comes from it, fed the same float32 samples in the same calls --
never from the device code.  Everything is compared with equality, after every call.

Rows sit n + PAD floats apart with 1e30 in the padding (a sample read beyond n would show in the
energy at once), and the first row starts 4 bytes past the allocation's 256-byte boundary.
"""
import functools
import os

import numpy as np
import pytest

import rds_clock_rows as rc

pytestmark = pytest.mark.gpu

PAD = 37
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _device(sdr, ctx, rows, cuts, bank=None, sync=None, **kw):
    """the bank over the cuts (every stream takes the same): per call (bits, state[, records, sync state])"""
    S, top = len(rows), max(max(cuts), 1)
    own = bank is None
    if own:
        bank = sdr.RdsClockBank(S, top, ctx=ctx, **kw)
    buf = sdr.DeviceBuffer(ctx, 4 * (S * (top + PAD) + 1))
    out, o = [], 0
    for n in cuts:
        m = np.full((S, n + PAD), 1e30, dtype=np.float32)
        for s, x in enumerate(rows):
            m[s, :n] = x[o:o + n]
        o += n
        buf.upload(m, offset=4)
        bank.process_dev(buf.ptr + 4, n, n + PAD)
        res = (bank.bits(), bank.state())
        if sync is not None:
            bank.feed(sync)
            res += (sync.blocks(), sync.state())
        out.append(res)
    buf.free()
    if own:
        bank.close()
    return out


def _check(sdr, rows, cuts, dev, **kw):
    for s, x in enumerate(rows):
        ref = rc.model_calls(sdr, x, cuts, **kw)
        for k, (bits, state) in enumerate(ref):
            np.testing.assert_array_equal(dev[k][0][s], bits, err_msg=f"stream {s}, call {k}")
            assert dev[k][1][s] == state, (s, k)


@functools.lru_cache(maxsize=None)
def _three():
    rows = [rc.row(ppm=1000, delay=5, sigma=0.3, seed=3), rc.row(ppm=-1000, delay=17, sigma=0.5, seed=6),
            rc.row(ppm=50, sigma=0.05, seed=7)]
    n = min(len(x) for x in rows)
    return tuple(x[:n] for x in rows)


def test_one_call(sdr, gpu_ctx):
    rows = _three()
    cuts = [len(rows[0])]
    dev = _device(sdr, gpu_ctx, rows, cuts)
    _check(sdr, rows, cuts, dev)
    assert dev[0][1][0][8] >= 6 and dev[0][1][1][8] >= 6          # both of the fast rows wrap


@pytest.mark.parametrize("seed", [1, 2])
def test_random_cuts(sdr, gpu_ctx, seed):
    rows = tuple(x[:60_000 * seed] for x in _three())
    cuts = rc.random_cuts(len(rows[0]) - 1000, seed, top=(3000, 9000)[seed - 1])
    cuts[3:3] = [1, 0, 766, 233]                                  # less than a segment, and up to its end
    assert 0 in cuts and sum(cuts) == len(rows[0]) and max(cuts) > 2 * 768
    _check(sdr, rows, cuts, _device(sdr, gpu_ctx, rows, cuts))


@functools.lru_cache(maxsize=None)
def _many(S, length):
    base = [rc.row(ppm=p, delay=d, sigma=sg, seed=10 + k, groups=7)
            for k, (p, d, sg) in enumerate(((1000, 20, 0.3), (-1000, 2, 0.3), (0, 9, 0.05), (300, 0, 0.8), (-700, 23, 0.5),
                                            (50, 12, 0.2), (900, 21, 1.5)))]
    return tuple(base[s % 7][41 * (s // 7):][:length] for s in range(S))


@pytest.mark.parametrize("window", [1, 4, 16])
@pytest.mark.parametrize("n", [767, 768, 769, 1536 + 5])
@pytest.mark.parametrize("S", [1, 70])
def test_stream_counts(sdr, gpu_ctx, S, n, window):
    total = 19 * 768 + 300
    rows = _many(S, total)
    assert all(len(x) == total for x in rows)
    cuts = [n] * (total // n) + [total % n]
    bank = sdr.RdsClockBank(S, n, window=window, ctx=gpu_ctx)
    first = _device(sdr, gpu_ctx, rows, cuts, bank=bank)
    _check(sdr, rows, cuts, first, window=window)
    bank.reset()
    assert bank.state() == [(0,) * 10] * S and all(len(b) == 0 for b in bank.bits())
    again = _device(sdr, gpu_ctx, rows, cuts, bank=bank)
    for a, b in zip(first, again):
        assert a[1] == b[1] and all(np.array_equal(p, q) for p, q in zip(a[0], b[0]))
    bank.close()


def test_hysteresis_and_inserted_symbol(sdr, gpu_ctx):
    rows = (rc.row(seed=3, insert_at=4001)[:150_000], rc.row(seed=3, insert_at=2002)[:150_000])
    cuts = [50_000] * 3
    for h in (0, 8, 40):
        dev = _device(sdr, gpu_ctx, rows, cuts, hysteresis=h)
        _check(sdr, rows, cuts, dev, hysteresis=h)
        if h == 8:
            assert [st[9] for st in dev[-1][1]] == [1, 1]


def test_non_finite(sdr, gpu_ctx):
    x = _three()[0][:40_000].copy()
    at = np.random.default_rng(2).choice(len(x), 400, replace=False)
    x[at[0::3]], x[at[1::3]], x[at[2::3]] = np.nan, np.inf, -np.inf
    rows = (x, np.full(len(x), np.nan, dtype=np.float32))
    cuts = [10_000] * 4
    _check(sdr, rows, cuts, _device(sdr, gpu_ctx, rows, cuts))


def test_chain_beside_the_link_bank(sdr, gpu_ctx):
    """RdsClockBank -> feed -> RdsSyncBank: the records equal the model chain's; on the +-500 ppm
    rows the clock path keeps at least 150 of the generator's 160 blocks where RdsLinkBank ->
    block_sync() on the same device rows, the whole row one call, loses at least a third."""
    rows = [rc.row(ppm=500, sigma=0.3, seed=3), rc.row(ppm=-500, sigma=0.3, seed=3)]
    n = min(len(x) for x in rows)
    rows = [x[:n] for x in rows]
    half = n // 2
    cuts = [half, n - half]
    bank = sdr.RdsClockBank(2, max(cuts), ctx=gpu_ctx)
    sync = bank.block_sync()
    assert sync.S == 2 and sync.max_bits == bank.max_bits == 17 * -(-max(cuts) // 768) + 1
    dev = _device(sdr, gpu_ctx, rows, cuts, bank=bank, sync=sync)
    _check(sdr, rows, cuts, dev)
    new = []
    for s, x in enumerate(rows):
        clk, model = sdr.RdsSymbolClock(), sdr.RdsBlockSync()
        rec, o = [], 0
        for k, c in enumerate(cuts):
            r = model.process(clk.process(x[o:o + c]))
            o += c
            assert dev[k][2][s] == r and dev[k][3][s] == model.state(), (s, k)
            rec += r
        new.append(rc.generator_blocks(rec, 3))
    # the link bank on the same rows
    buf = sdr.DeviceBuffer.from_array(gpu_ctx, np.stack(rows))
    link = sdr.RdsLinkBank(2, n, ctx=gpu_ctx)
    lsync = link.block_sync()
    link.process_dev(buf.ptr, n, n)
    lsync.process_links(link)
    old = [rc.generator_blocks(r, 3) for r in lsync.blocks()]
    print("generator blocks of 160: clock path", new, "link bank path", old)
    for obj in (lsync, link, sync, bank):
        obj.close()
    buf.free()
    assert min(new) >= 150
    assert max(old) <= 160 * 2 // 3


NBLK, B = 48, 153_600
LATE = 295                          # IQ samples: 7 samples of rrc_i


def test_through_the_receiver(sdr, gpu_ctx):
    """u8 IQ with coded groups through Receiver -> rds_clock() -> block_sync(), beside rds_link() ->
    block_sync() on the same rrc_i rows, 48 blocks of 153 600: captures at clock_ppm 0, +100 and -100,
    and the 0 ppm capture started 295 samples late.  The device clock equals the model on the fetched
    rows exactly, block by block, on all four.

    What one MI355X gave (block records of status 0 / 1 / 2; 140 blocks are complete in 48 blocks):

        capture               clock path     link-bank path
        0 ppm                 140 / 0 / 0    91 / 41 / 5
        +100 ppm              140 / 0 / 0    77 / 33 / 26
        -100 ppm              140 / 0 / 0    61 / 13 / 63
        0 ppm, 295 late       140 / 0 / 0    139 / 0 / 0

    The link-bank path is erratic at 0 ppm already: its offset is the first maximum of the first 24
    samples of a filter transient (23 on the plain capture, where the symbol energy peaks at 6), and
    started 253 or 337 samples late the same capture gave it 46 / 5 / 86.  The clock path gave 139 or
    140 error-free blocks at every start tried, phi constant over the 48 blocks at 0 ppm and 16 steps
    one way at +-100 ppm, so the receiver's RDS PLL holds the carrier at that offset over 3 s.  The
    0 ppm comparison with the link-bank path -- status-0 blocks within 2 -- is therefore made on the
    late capture, where that path's fixed offset is a working one; the plain capture can only show
    that the clock path loses nothing (it has every block).  All counts go to
    profiles/rdsclock/e2e.txt, recorded and not asserted."""
    cases = (("0 ppm", 0, 0), ("+100 ppm", 100, 0), ("-100 ppm", -100, 0), (f"0 ppm, {LATE} late", 0, LATE))
    iq = [sdr.synth.fm_iq(NBLK * B + late, seed=31, dtype=np.uint8, rds_groups=True, clock_ppm=p)[2 * late:] for _, p, late in cases]
    S = len(cases)
    rx = sdr.Receiver(S, B, mono=False, rds=True, iq_dtype=np.uint8, ctx=gpu_ctx)
    clock, link = rx.rds_clock(), rx.rds_link()
    csync, lsync = clock.block_sync(), link.block_sync()
    models = [sdr.RdsSymbolClock() for _ in cases]
    got = np.zeros((2, S, 3), dtype=np.int64)                     # path, stream, status
    for k in range(NBLK):
        buf = sdr.DeviceBuffer.from_array(gpu_ctx, np.stack([x[2 * k * B:2 * (k + 1) * B] for x in iq]))
        rx.process_dev(buf.ptr, B)
        clock.process_rx(rx)
        clock.feed(csync)
        link.process_rx(rx)
        lsync.process_links(link)
        bits, state = clock.bits(), clock.state()
        rrc = rx.output("rrc_i")
        for s in range(S):
            np.testing.assert_array_equal(bits[s], models[s].process(rrc[s]), err_msg=f"stream {s}, block {k}")
            assert state[s] == models[s].state(), (s, k)
        for path, sync in enumerate((csync, lsync)):
            for s, rec in enumerate(sync.blocks()):
                for r in rec:
                    got[path, s, r[2]] += 1
        buf.free()
    lines = [f"{NBLK} blocks of {B} u8 IQ samples, coded groups (seed 31); block records by status 0 / 1 / 2",
             f"{'capture':20s}   Receiver.rds_clock -> block_sync   Receiver.rds_link -> block_sync   phi; steps fwd / back, wraps"]
    for s, (name, _, _) in enumerate(cases):
        st = models[s].state()
        lines.append(f"{name:20s}   {got[0, s].tolist()!s:33s}   {got[1, s].tolist()!s:32s}   {st[2]}; {st[6]} / {st[7]}, {st[8]}")
    print("\n".join(lines))
    try:
        os.makedirs(os.path.join(ROOT, "profiles", "rdsclock"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "rdsclock", "e2e.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass
    for obj in (csync, lsync, clock, link, rx):
        obj.close()
    assert abs(int(got[0, 3, 0]) - int(got[1, 3, 0])) <= 2 and got[0, 3, 0] >= 130
    assert got[0, 0, 0] >= got[1, 0, 0] - 2


def test_arguments(sdr, gpu_ctx):
    bank = sdr.RdsClockBank(2, 1000, ctx=gpu_ctx)
    assert bank.max_bits == 17 * 2 + 1 and (bank.window, bank.hysteresis) == (4, 8)
    buf = sdr.DeviceBuffer(gpu_ctx, 4 * 2 * 1040 + 16)
    buf.zero()
    for kw in (dict(window=0, hysteresis=8), dict(window=17, hysteresis=8), dict(window=4, hysteresis=-1),
               dict(window=4, hysteresis=(1 << 20) + 1)):
        with pytest.raises(ValueError):
            bank.set_params(**kw)
        with pytest.raises(ValueError):
            sdr.RdsClockBank(1, 100, ctx=gpu_ctx, **kw)
    for n, stride in ((1001, 1040), (-1, 1040), (1000, 999)):
        with pytest.raises(ValueError):
            bank.process_dev(buf.ptr, n, stride)
    with pytest.raises(ValueError):
        bank.process_dev(0, 1000, 1000)
    with pytest.raises(ValueError):
        bank.process_dev(buf.ptr + 2, 1000, 1000)                 # not aligned to 4 bytes
    for bad in (dict(nstreams=0, max_n=100), dict(nstreams=1, max_n=0), dict(nstreams=1, max_n=(1 << 24) + 1)):
        with pytest.raises(ValueError):
            sdr.RdsClockBank(ctx=gpu_ctx, **bad)
    bank.process_dev(buf.ptr, 0, 0)                               # the limits themselves are legal
    bank.process_dev(buf.ptr + 4, 1000, 1040)
    assert bank.state() == [(768, 1, 0, 0, 32, 16, 0, 0, 0, 0)] * 2 and [len(b) for b in bank.bits()] == [15, 15]
    three = sdr.RdsSyncBank(3, bank.max_bits, ctx=gpu_ctx)
    with pytest.raises(ValueError):
        bank.feed(three)
    small = sdr.RdsSyncBank(2, bank.max_bits - 1, ctx=gpu_ctx)
    with pytest.raises(ValueError):
        bank.feed(small)
    ok = bank.block_sync(max_burst=5, lose_after=3)
    assert (ok.max_burst, ok.lose_after, ok.ctx, ok.max_bits) == (5, 3, bank.ctx, bank.max_bits)
    bank.feed(ok)
    assert ok.state() == [(0, 0, 0, 0, 0, 0, 0)] * 2
    rx = sdr.Receiver(1, 51200, mono=True, rds=False, ctx=gpu_ctx)
    with pytest.raises(ValueError):
        rx.rds_clock()
    for obj in (rx, ok, small, three, bank):
        obj.close()
    buf.free()
