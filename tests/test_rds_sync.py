"""Device-side RDS block sync (RdsSyncBank, csrc/rds_sync.hip) against the host model.

rtsdr.RdsBlockSync is the specification (tests/test_rds_sync_model.py pins it on the CPU against
hand-built streams and the link-layer fixture): every expected record, state and counter here
comes from it, fed the same bits in the same calls -- never from the device code.  Everything is
compared with equality, after every call.

One accepted link event need not be a block record: the link layer's frame rule accepts the first
syndrome match it meets, whatever surrounds it, and the sync rule acquires only on two offset
syndromes 26 bits apart in consecutive slots.  On the noisy row (seed 13, sigma 1.0) the link
layer accepts exactly one match, a chance one with no such neighbour on either side, and the
model never acquires.  test_through_the_link_bank therefore asserts, for every accepted event:
it is a status-0 record with the same type, position and word, or neither window 26 bits from
it has an offset syndrome of the neighbouring slot (so no acquisition rule could have used it);
on the clean rows (seeds 5, 7, the shifted one) all 19 / 19 / 2 accepted events are records.
"""
import functools

import numpy as np
import pytest

import rds_sync_streams as rs

pytestmark = pytest.mark.gpu

NBITS = 3800                        # 146 blocks: an acquisition, two full rounds of 64 and a partial one
PAD = 40
BLOCK = 3648
NSYM = 8 * 152
PULSE = np.sin(np.pi * (np.arange(24) + 0.5) / 24)


def _fit(bits, seed, n=NBITS):
    """exactly n bits: cut, or seeded random bits appended"""
    tail = np.random.default_rng(2000 + seed).integers(0, 2, max(n - len(bits), 0)).tolist()
    return (list(bits) + [int(b) for b in tail])[:n]


@functools.lru_cache(maxsize=None)
def _streams():
    import rtsdr as sdr
    g = [rs.groups(20 + k, 37, vb) for k, vb in enumerate((False, None, True, None, None))]
    s = []
    # 0: clean groups from bit 0 on
    s.append(rs.coded(sdr, g[0], 0))
    # 1: 27 junk bits; every correction case (single bits, bursts of 2 .. 5) on blocks 3, 5, 7, ...
    b = rs.coded(sdr, g[1], 27, seed=1)
    for k, offs in enumerate(rs.correction_cases()):
        b = rs.flip(b, 3 + 2 * k, offs, 27)
    s.append(b)
    # 2: version-B groups behind 1 junk bit: damaged C' blocks behind clean, corrected and
    # uncorrectable B blocks, at lane 0 of a round (block 66) among them
    b = rs.coded(sdr, g[2], 1, seed=2)
    for blk, b_offs in ((6, []), (14, [7]), (22, rs.UNCORRECTABLE), (66, []), (130, [3]), (134, rs.UNCORRECTABLE)):
        b = rs.flip(rs.flip(b, blk, [20], 1), blk - 1, b_offs, 1)
    b = rs.flip(b, 29, rs.UNCORRECTABLE, 1)             # an undamaged C' behind an uncorrectable B
    s.append(b)
    # 3: 25 junk bits; a 12-block loss over blocks 60 .. 71 (lanes 58 .. 63 and 0 .. 5 of the
    # rounds from block 2 on), eleven bad blocks that keep sync, and a loss over bit 3000
    b = rs.coded(sdr, g[3], 25, seed=3)
    b = rs.bad_run(rs.bad_run(rs.bad_run(b, 60, 12, 25), 84, 11, 25), 109, 12, 25)
    s.append(b)
    # 4: 26 junk bits; seven extra bits in front of block 70
    s.append(rs.slipped(rs.coded(sdr, g[4], 26, seed=4), 26 + 26 * 70))
    out = tuple(np.array(_fit(b, k), dtype=np.uint8) for k, b in enumerate(s))
    for b in out:
        b.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _noisy_streams():
    import rtsdr as sdr
    return tuple(np.array(rs.noisy(sdr, seed, 20_000, ber), dtype=np.uint8) for seed, ber in ((7, 0.035), (12, 0.08)))


def _device(sdr, ctx, streams, cuts, sync=None, counts=True, **kw):
    """the bank over per-stream cuts: per call ([records per stream], [state per stream]).  Rows
    are n + PAD apart with 0xFF in the padding and behind a stream's own count; bits 1 .. 7 of a
    byte are set on the odd streams."""
    S = len(streams)
    ncall = max(len(c) for c in cuts)
    cuts = [list(c) + [0] * (ncall - len(c)) for c in cuts]
    top = max(max(c) for c in cuts)
    own = sync is None
    if own:
        sync = sdr.RdsSyncBank(S, max(top, 1), ctx=ctx, **kw)
    buf = sdr.DeviceBuffer(ctx, S * (top + PAD) + 16)
    cbuf = sdr.DeviceBuffer(ctx, 4 * S + 16)
    out, o = [], [0] * S
    for k in range(ncall):
        cnt = [cuts[s][k] for s in range(S)]
        n = max(cnt)
        m = np.full((S, n + PAD), 0xFF, dtype=np.uint8)
        for s, b in enumerate(streams):
            m[s, :cnt[s]] = b[o[s]:o[s] + cnt[s]] | (0xA4 if s & 1 else 0)
            o[s] += cnt[s]
        buf.upload(m)
        if counts:
            cbuf.upload(np.array(cnt, dtype=np.int32))
        else:
            assert all(c == n for c in cnt)
        sync.process_dev(buf.ptr, n, n + PAD, cbuf.ptr if counts else 0)
        out.append((sync.blocks(), sync.state()))
    buf.free()
    cbuf.free()
    if own:
        sync.close()
    assert all(o[s] == len(b) for s, b in enumerate(streams))
    return out


def _check(sdr, streams, cuts, dev, **kw):
    """records, state and counters of every stream after every call; returns the models' final states"""
    final = []
    for s, b in enumerate(streams):
        ref = rs.model_calls(sdr, b.tolist(), cuts[s], **kw)
        for k, (rec, state) in enumerate(ref):
            assert dev[k][0][s] == rec, (s, k)
            assert dev[k][1][s] == state, (s, k)
        for k in range(len(ref), len(dev)):                      # calls that brought this stream nothing
            assert dev[k][0][s] == [] and dev[k][1][s] == ref[-1][1], (s, k)
        final.append(ref[-1][1])
    return final


def test_streams_are_what_they_claim(sdr):
    """the model on the hand-built streams: the conditions the device tests lean on (no GPU work)"""
    st = [rs.model_calls(sdr, b.tolist(), [len(b)])[0] for b in _streams()]
    assert all(len(b) == NBITS and NBITS // 26 >= 130 for b in _streams())
    assert st[0][1][2:] == (146, 0, 0, 1, 0) and st[0][0][0][1] == 0
    assert st[1][0][0][1] == 27 and st[1][1][3:] == (26 + 3, 24, 1, 0)
    assert [r[0] for r in st[2][0][:4]] == [0, 1, 4, 3] and st[2][0][0][1] == 1
    by_pos = {r[1]: r for r in st[2][0]}
    assert [by_pos[1 + 26 * k][2] for k in (6, 14, 22, 66, 130, 134)] == [1, 1, 2, 1, 1, 2]
    assert [by_pos[1 + 26 * k][0] for k in (6, 14, 22, 66, 130, 134, 30)] == [4, 4, 2, 4, 4, 2, 4]
    assert st[3][1][5:] == (3, 2) and st[3][1][0] == 1
    lost = [r[1] for r in st[3][0] if r[2] == 2]
    assert 25 + 26 * 71 in lost and 25 + 26 * 94 in lost and 25 + 26 * 120 in lost
    assert 25 + 26 * 109 < 3000 < 25 + 26 * 121
    assert st[4][1][5:] == (2, 1) and st[4][0][-1][1] % 26 == (26 + 7) % 26
    for rec, state in st:
        pos = [r[1] for r in rec]
        assert all(b > a for a, b in zip(pos, pos[1:]))


def test_one_call(sdr, gpu_ctx):
    streams = _streams()
    cuts = [[NBITS]] * len(streams)
    _check(sdr, streams, cuts, _device(sdr, gpu_ctx, streams, cuts, counts=False))


@pytest.mark.parametrize("max_burst,lose_after", [(0, 12), (1, 3), (5, 1), (5, 255)])
def test_parameters(sdr, gpu_ctx, max_burst, lose_after):
    streams = _streams()
    cuts = [rs.cuts_of(NBITS, 1000)] * len(streams)
    kw = dict(max_burst=max_burst, lose_after=lose_after)
    _check(sdr, streams, cuts, _device(sdr, gpu_ctx, streams, cuts, **kw), **kw)


@pytest.mark.parametrize("size", [1, 25, 26, 27, 63, 64, 65, 257, 1000])
def test_equal_calls(sdr, gpu_ctx, size):
    streams = _streams()
    cuts = [rs.cuts_of(NBITS, size)] * len(streams)
    _check(sdr, streams, cuts, _device(sdr, gpu_ctx, streams, cuts))


@pytest.mark.parametrize("seed", [1, 2])
def test_random_cuts_with_counts_and_reset(sdr, gpu_ctx, seed):
    """Every stream has its own random cuts, empty ones among them, so one call brings different
    counts; after reset() the same calls give the same results."""
    streams = _streams()
    cuts = [rs.random_cuts(NBITS, 10 * seed + s, top=(40, 300)[seed - 1]) for s in range(len(streams))]
    ncall = max(len(c) for c in cuts)
    assert any(len({(c + [0] * ncall)[k] for c in cuts}) > 2 and 0 in [(c + [0] * ncall)[k] for c in cuts] for k in range(ncall))
    sync = sdr.RdsSyncBank(len(streams), 300, ctx=gpu_ctx)
    first = _device(sdr, gpu_ctx, streams, cuts, sync=sync)
    _check(sdr, streams, cuts, first)
    sync.reset()
    assert sync.state() == [(0, 0, 0, 0, 0, 0, 0)] * len(streams) and sync.blocks() == [[]] * len(streams)
    assert _device(sdr, gpu_ctx, streams, cuts, sync=sync) == first
    sync.close()


@pytest.mark.parametrize("cuts", ["one", 1000, "random"])
def test_bit_errors(sdr, gpu_ctx, cuts):
    """Coded groups with seeded bit errors at 3.5 % and 8 % over 20 000 bits: the model loses and
    finds sync at least three times on each."""
    streams = _noisy_streams()
    n = len(streams[0])
    c = {"one": [[n]] * 2, 1000: [rs.cuts_of(n, 1000)] * 2, "random": [rs.random_cuts(n, 30 + s, top=2500) for s in range(2)]}[cuts]
    final = _check(sdr, streams, c, _device(sdr, gpu_ctx, streams, c))
    for state in final:
        assert state[5] >= 3 and state[6] >= 3, state


def _row(seed, nsym=NSYM, sigma=0.3):
    """a half-sine row as in tests/test_rds_links.py"""
    import rtsdr
    s = rtsdr.synth.rds_symbols(nsym // 2 + 2, seed)[:nsym]
    x = (s[:, None] * PULSE).ravel()
    x += np.random.default_rng(seed + 100).normal(0, sigma, len(x))
    return x.astype(np.float32)


def link_expect(sdr, x, cuts):
    """The host link layer and the model over the cuts of one row: per call None where the host
    layer raised (the device's FAULT: no bits), else dict(host=its result, rec=the model's
    records on the call's new bits, state=the model's state, accepted=[(type, position, word)])."""
    from rtsdr import rdssync
    link, model = sdr.RdsLinkLayer(), sdr.RdsBlockSync()
    out, o, pp, first = [], 0, 0, True
    for n in cuts:
        try:
            r = link.process(np.asarray(x[o:o + n], dtype=np.float64))
        except ValueError:
            out.append(None)
            o += n
            continue
        o += n
        d = r["diff"]
        new = d if first else d[27:]
        first = False
        acc = []
        for t, p, ok in r["events"]:
            if ok:
                w = int("".join(str(b) for b in d[p - pp:p - pp + 26]), 2)
                assert rdssync.syndrome(w) == rdssync.SYNDROMES["ABCD"[t]]
                acc.append((t, p, w >> 10))
        pp += len(d) - 27
        out.append(dict(host=r, rec=model.process(new), state=model.state(), accepted=acc, nbits=model.nbits))
    link.close()
    return out


def isolated(bits, t, p):
    """no window 26 bits from p has an offset syndrome of the slot next to type t's"""
    from rtsdr import rdssync
    slot_of = {rdssync.SYNDROMES[name]: (0, 1, 2, 3, 2)[k] for k, name in enumerate(rdssync.TYPE_NAMES)}
    for q, want in ((p - 26, (t - 1) & 3), (p + 26, (t + 1) & 3)):
        if q >= 0 and q + 26 <= len(bits):
            s = rdssync.syndrome(int("".join(str(b) for b in bits[q:q + 26]), 2))
            if slot_of.get(s) == want:
                return False
    return True


def check_accepted(expect):
    """every accepted link event of one stream is a status-0 record, or isolated; returns (accepted, records among them)"""
    calls = [e for e in expect if e is not None]
    bits = np.concatenate([e["host"]["diff"] if k == 0 else e["host"]["diff"][27:] for k, e in enumerate(calls)])
    good = {(r[0], r[1], r[3]) for e in calls for r in e["rec"] if r[2] == 0}
    acc = [a for e in calls for a in e["accepted"]]
    for a in acc:
        assert a in good or isolated(bits, a[0], a[1]), a
    return len(acc), sum(a in good for a in acc)


@pytest.mark.parametrize("n", [BLOCK, 7 * BLOCK])
def test_through_the_link_bank(sdr, gpu_ctx, n):
    """Half-sine rows through RdsLinkBank.process_dev and process_links, in the reference's blocks
    and as one call: the records equal the model on the host link layer's new bits, and the link
    bank's own outputs equal those of a bank with no sync attached."""
    rows = [_row(5), _row(7), _row(13, sigma=1.0), _row(5)[24:]]
    total = min(len(x) for x in rows) // n * n
    cuts = [n] * (total // n)
    expect = [link_expect(sdr, x, cuts) for x in rows]
    S = len(rows)
    bank, plain = sdr.RdsLinkBank(S, n, ctx=gpu_ctx), sdr.RdsLinkBank(S, n, ctx=gpu_ctx)
    sync = bank.block_sync()
    assert sync.S == S and sync.max_bits == n // 24 // 2
    o = 0
    for k in range(len(cuts)):
        buf = sdr.DeviceBuffer.from_array(gpu_ctx, np.stack([x[o:o + n] for x in rows]))
        bank.process_dev(buf.ptr, n, n)
        sync.process_links(bank)
        plain.process_dev(buf.ptr, n, n)
        ev, status = bank.events()
        ev2, status2 = plain.events()
        assert ev == ev2 and np.array_equal(status, status2) and np.array_equal(bank.counts, plain.counts)
        blocks, state = sync.blocks(), sync.state()
        for s in range(S):
            e = expect[s][k]
            assert [v[:3] for v in ev[s]] == e["host"]["events"]
            for a, b in zip(bank.bits(s), plain.bits(s)):
                np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(bank.bits(s)[1], e["host"]["diff"])
            assert blocks[s] == e["rec"], (s, k)
            assert state[s] == e["state"], (s, k)
        buf.free()
        o += n
    counts = [check_accepted(e) for e in expect]
    assert counts[0] == (19, 19) and counts[1] == (19, 19) and counts[3] == (2, 2)
    assert counts[2][0] >= 1                                      # the noisy row: see the module docstring
    for b in (sync, bank, plain):
        b.close()


def test_link_fault_adds_no_bits(sdr, gpu_ctx):
    """NaN at sample 3 of stream 1's first call: the link bank faults that stream, the sync takes
    no bits for it in that call and is the model on the later calls' bits; streams 0 and 2 are
    untouched."""
    bad = _row(7).copy()
    bad[3] = np.nan
    rows = [_row(5), bad, _row(9)]
    cuts = [BLOCK] * (len(bad) // BLOCK)
    expect = [link_expect(sdr, x, cuts) for x in rows]
    assert expect[1][0] is None and all(e is not None for e in expect[1][1:])
    bank = sdr.RdsLinkBank(3, BLOCK, ctx=gpu_ctx)
    sync = bank.block_sync()
    acquired = 0
    for k in range(len(cuts)):
        buf = sdr.DeviceBuffer.from_array(gpu_ctx, np.stack([x[k * BLOCK:(k + 1) * BLOCK] for x in rows]))
        bank.process_dev(buf.ptr, BLOCK, BLOCK)
        sync.process_links(bank)
        ev, status = bank.events()
        blocks, state = sync.blocks(), sync.state()
        for s in range(3):
            e = expect[s][k]
            if e is None:
                assert status[s] & sdr.RdsLinkBank.FAULT and blocks[s] == [] and state[s] == (0, 0, 0, 0, 0, 0, 0)
            else:
                assert status[s] == 0 and blocks[s] == e["rec"] and state[s] == e["state"], (s, k)
        acquired += len(blocks[1])
        buf.free()
    assert acquired >= 20
    sync.close()
    bank.close()


def test_receiver_end_to_end(sdr, gpu_ctx, golden):
    """The golden file's u8 IQ and two more seeds through Receiver -> rds_link() -> block_sync():
    the records equal the model on the host layer's bits of the fetched rrc_i rows; stream 0 gives
    20 blocks of which the reference rule accepts 2, at least 18 with the generator's words."""
    z = golden("rds_link.npz")
    nblk, B = len(z["rrc_i"]), 153_600
    seed = int(z["seed"])
    iq = [sdr.synth.fm_iq(nblk * B, seed=sd, dtype=np.uint8, rds_groups=True) for sd in (seed, seed + 1, seed + 2)]
    iq[0] = sdr.synth.fm_iq(int(z["n_complex"]), seed=seed, dtype=np.uint8, rds_groups=True)[:2 * nblk * B]
    rx = sdr.Receiver(3, B, mono=False, rds=True, iq_dtype=np.uint8, ctx=gpu_ctx)
    bank = rx.rds_link()
    sync = bank.block_sync()
    links = [sdr.RdsLinkLayer() for _ in range(3)]
    models = [sdr.RdsBlockSync() for _ in range(3)]
    prog = [sdr.RdsProgramme() for _ in range(3)]
    records, accepted = [[] for _ in range(3)], []
    for k in range(nblk):
        buf = sdr.DeviceBuffer.from_array(gpu_ctx, np.stack([x[2 * k * B:2 * (k + 1) * B] for x in iq]))
        rx.process_dev(buf.ptr, B)
        bank.process_rx(rx)
        sync.process_links(bank)
        ev, status = bank.events()
        blocks, state = sync.blocks(), sync.state()
        rrc = rx.output("rrc_i")
        for s in range(3):
            d = links[s].process(rrc[s])["diff"]
            rec = models[s].process(d if k == 0 else d[27:])
            assert blocks[s] == rec and state[s] == models[s].state(), (s, k)
            records[s] += blocks[s]
            prog[s].feed(blocks[s])
        accepted += [e for e in ev[0] if e[2]]
        buf.free()
    rng = np.random.default_rng(seed)
    gen = [int(rng.integers(0, 1 << 16)) for _ in range(20)]
    first = records[0][:20]
    assert len(first) == 20 and [r[1] for r in first] == [first[0][1] + 26 * k for k in range(20)]
    assert sum(r[3] == w and r[2] <= 1 for r, w in zip(first, gen)) >= 18
    assert len([e for e in accepted if e[1] <= first[-1][1]]) == 2
    assert prog[0].groups >= 4 and prog[0].pi in gen[0::4]         # random groups: every A word is another "PI"
    for obj in (sync, bank, rx, *links):
        obj.close()


def test_arguments(sdr, gpu_ctx):
    sync = sdr.RdsSyncBank(2, 1000, ctx=gpu_ctx)
    buf = sdr.DeviceBuffer(gpu_ctx, 2 * 1040)
    buf.zero()
    for kw in (dict(max_burst=6, lose_after=12), dict(max_burst=-1, lose_after=12), dict(max_burst=2, lose_after=0),
               dict(max_burst=2, lose_after=256)):
        with pytest.raises(ValueError):
            sync.set_params(**kw)
        with pytest.raises(ValueError):
            sdr.RdsSyncBank(1, 100, ctx=gpu_ctx, **kw)
    for n, stride in ((1001, 1040), (-1, 1040), (1000, 999)):
        with pytest.raises(ValueError):
            sync.process_dev(buf.ptr, n, stride)
    with pytest.raises(ValueError):
        sync.process_dev(0, 1000, 1000)
    for bad in (dict(nstreams=0, max_bits=100), dict(nstreams=1, max_bits=0)):
        with pytest.raises(ValueError):
            sdr.RdsSyncBank(ctx=gpu_ctx, **bad)
    sync.process_dev(buf.ptr, 1000, 1040)            # the limits themselves are legal
    sync.process_dev(buf.ptr, 0, 0)
    assert sync.state() == [(0, 0, 0, 0, 0, 0, 0)] * 2 and sync.blocks() == [[], []]
    # process_links: the stream counts, the contexts and the sizes must agree
    bank = sdr.RdsLinkBank(3, 4000, ctx=gpu_ctx)
    with pytest.raises(ValueError):
        sync.process_links(bank)
    small = sdr.RdsSyncBank(3, 10, ctx=gpu_ctx)
    with pytest.raises(ValueError):
        small.process_links(bank)
    from rtsdr import _lib
    other = sdr.Context(_lib.default_device())
    far = sdr.RdsSyncBank(3, 4000, ctx=other)
    with pytest.raises(ValueError):
        far.process_links(bank)
    far.close()
    other.close()
    ok = bank.block_sync(max_burst=5, lose_after=3)
    assert (ok.max_burst, ok.lose_after, ok.ctx) == (5, 3, bank.ctx)
    for obj in (ok, small, bank, sync):
        obj.close()
    buf.free()
