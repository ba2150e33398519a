"""Device-side RDS link layer (RdsLinkBank, csrc/rds.hip) against the host layer.

The host RdsLinkLayer is the specification (tests/test_rds_link.py pins it to the reference
script's own prints): every expected value here comes from it, fed the same float32 rows widened
to float64 -- never from the device code.  Compared with equality: the Manchester bits, the
scanned row and the events of every stream and every call.  Event words are checked against the
host's scanned row: with pp the position at a call's entry and d that call's row, an event at
position p carries int(d[p - pp : p - pp + 16]), and pp += len(d) - 27 after each call.

Rows: coded RDS groups (synth.rds_symbols) as half-sine symbols of 24 samples plus noise.  The
reference's clock recovery is crude, so many rows give few accepted events; the equality of
every bit is the weight-bearing check, and the conditions asserted per case (event counts, both
start positions, tie counts, a RESYNC) keep the event checks from being vacuous.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NSYM = 8 * 152                      # 29 184 samples: eight of the reference's RDS blocks of 3648
BLOCK = 3648
PULSE = np.sin(np.pi * (np.arange(24) + 0.5) / 24)


@functools.lru_cache(maxsize=None)
def _row(seed, nsym=NSYM, sigma=0.3):
    import rtsdr
    s = rtsdr.synth.rds_symbols(nsym // 2 + 2, seed)[:nsym]
    x = (s[:, None] * PULSE).ravel()
    x += np.random.default_rng(seed + 100).normal(0, sigma, len(x))
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def _half(x):
    """rounded to multiples of 0.5: hundreds of equal symbol pairs, repeated values in a row's tail"""
    y = (np.round(x.astype(np.float64) * 2) / 2).astype(np.float32)
    y.setflags(write=False)
    return y


def _cuts(total, n):
    return [n] * (total // n)


def _host(sdr, x, cuts, resync=0):
    """the host layer over the cuts of one row: per call its result dict, or None where it raised"""
    link = sdr.RdsLinkLayer(resync_after=resync)
    out, o = [], 0
    for n in cuts:
        try:
            out.append(link.process(np.asarray(x[o:o + n], dtype=np.float64)))
        except ValueError:
            out.append(None)
        o += n
    link.close()
    return out


def _device(sdr, ctx, rows, cuts, pad=0, fill=1e30, bank=None, **kw):
    """the bank over the same cuts of all rows: per call (events, status, counts, [(bits, diff)])"""
    S = len(rows)
    own = bank is None
    if own:
        bank = sdr.RdsLinkBank(S, max(cuts), ctx=ctx, **kw)
    out, o = [], 0
    for n in cuts:
        stride = n + pad
        m = np.full((S, stride), fill, dtype=np.float32)
        for s, x in enumerate(rows):
            m[s, :n] = x[o:o + n]
        buf = sdr.DeviceBuffer.from_array(ctx, m)
        bank.process_dev(buf.ptr, n, stride)
        ev, status = bank.events()
        out.append((ev, status, bank.counts.copy(), [bank.bits(s) for s in range(S)]))
        buf.free()
        o += n
    if own:
        bank.close()
    return out


def _check_stream(dev, host, s):
    """bits, scanned bits, events and event words of stream s, call by call; returns its events"""
    pp, events = 0, []
    for call, (got, ref) in enumerate(zip(dev, host)):
        ev, status, counts, bd = got
        assert ref is not None, "the host layer raised: compare this call by hand"
        assert status[s] == 0, (s, call, status)
        np.testing.assert_array_equal(bd[s][0], ref["bits"], err_msg=f"bits, stream {s}, call {call}")
        np.testing.assert_array_equal(bd[s][1], ref["diff"], err_msg=f"diff, stream {s}, call {call}")
        assert [e[:3] for e in ev[s]] == ref["events"], (s, call)
        assert counts[s] == len(ref["events"])
        d = ref["diff"]
        for t, p, ok, word in ev[s]:
            if t == 4:
                assert word == 0
            else:
                assert word == int("".join(str(b) for b in d[p - pp:p - pp + 16]), 2), (s, call, p)
        pp += len(d) - 27
        events += ev[s]
    return events


def _compare(sdr, ctx, rows, cuts, **kw):
    resync = kw.get("resync_after", 0)
    dev = _device(sdr, ctx, rows, cuts, **kw)
    return [_check_stream(dev, _host(sdr, x, cuts, resync), s) for s, x in enumerate(rows)]


def _info_words(seed, count):
    rng = np.random.default_rng(seed)
    return [int(rng.integers(0, 1 << 16)) for _ in range(count)]


@pytest.mark.parametrize("n", [BLOCK, NSYM * 24])
def test_reference_blocks_and_one_call(sdr, gpu_ctx, n):
    """Seeds 5 and 7 in the reference's blocks of 3648 and as one call: 23-24 events, 22 accepted,
    the accepted words a contiguous run of the generator's information words, >= 4 groups."""
    rows = [_row(5), _row(7)]
    for seed, ev in zip((5, 7), _compare(sdr, gpu_ctx, rows, _cuts(len(rows[0]), n))):
        acc = [e for e in ev if e[2]]
        assert 23 <= len(ev) <= 24 and len(acc) == 22, (len(ev), len(acc))
        words = [e[3] for e in acc]
        gen = _info_words(seed, NSYM // 52 + 4)
        assert any(words == gen[k:k + len(words)] for k in range(len(gen) - len(words) + 1))
        groups = sdr.rds_groups(ev)
        assert len(groups) >= 4
        assert all(any(list(g) == gen[k:k + 4] for k in range(0, len(gen) - 3, 4)) for g in groups)


@pytest.mark.parametrize("n", [1536, 1543, 2000])
def test_offsets_that_walk(sdr, gpu_ctx, n):
    """The minimum call and calls with n % 24 != 0, where the value search moves the offset."""
    rows = [_row(5), _row(7)]
    for ev in _compare(sdr, gpu_ctx, rows, _cuts(len(rows[0]), n)):
        assert len(ev) >= 1


def _screen(sym):
    """the block-0 screening restated from the host layer's block-0 symbols"""
    c0 = c1 = 0
    for m in range(len(sym) // 4):
        a, b, c = sym[2 * m], sym[2 * m + 1], sym[2 * m + 2]
        if (a > 0 and b > 0) or (a < 0 and b < 0):
            c0 += 1
        elif (b > 0 and c > 0) or (b < 0 and c < 0):
            c1 += 1
    return 1 if c0 > c1 else 0


def test_start_position_one_and_ties(sdr, gpu_ctx):
    """Rows with the first 24 samples dropped and rows rounded to multiples of 0.5: both start
    positions occur, and at least one row has >= 100 tied symbol pairs."""
    rows = [_row(5), _row(7), _row(5)[24:], _row(7)[24:], _half(_row(5)), _half(_row(7)),
            _half(_row(5))[24:], _half(_row(7))[24:]]
    total = min(len(x) for x in rows)
    cuts = _cuts(total, BLOCK)
    _compare(sdr, gpu_ctx, rows, cuts)
    sps, ties = set(), []
    for x in rows:
        host = _host(sdr, x, cuts)
        sp = _screen(host[0]["symbols"])
        sps.add(sp)
        t = 0
        for r in host:
            s = r["symbols"]
            k = np.arange(len(s) // 2 - sp)
            t += int(np.sum(s[2 * k + sp] == s[2 * k + 1 + sp]))
        ties.append(t)
    assert sps == {0, 1}
    assert max(ties) >= 100, ties


def test_many_streams_with_stride(sdr, gpu_ctx):
    """Five different streams in one call, rows n + 40 apart with 1e30 in the padding: a read
    past n changes bits."""
    rows = [_row(5), _row(7)[24:], _half(_row(11)), _row(13, sigma=1.0), _half(_row(5))[24:]]
    total = min(len(x) for x in rows)
    _compare(sdr, gpu_ctx, rows, _cuts(total, 2000), pad=40)
    _compare(sdr, gpu_ctx, rows, [total], pad=40)


def test_span_length_row(sdr, gpu_ctx):
    """One stream of 64 x 3648 samples in one call, in calls of 3648, and as stream 2 of 3: each
    equals the host layer on that cut, whatever the other streams are."""
    x = _row(21, nsym=64 * 152)
    n = len(x)
    assert n == 64 * BLOCK
    one = _compare(sdr, gpu_ctx, [x], [n])[0]
    cut = _compare(sdr, gpu_ctx, [x], _cuts(n, BLOCK))[0]
    three = _compare(sdr, gpu_ctx, [_row(22, nsym=64 * 152), _half(_row(23, nsym=64 * 152)), x], [n])[2]
    assert three == one
    assert len(one) >= 1 and len(cut) >= 1


def test_resync(sdr, gpu_ctx):
    """resync_after=2 on noisy rows: the events, RESYNC events included, equal the host layer's."""
    rows = [_row(5, sigma=1.0), _row(7, sigma=1.0)]
    evs = _compare(sdr, gpu_ctx, rows, _cuts(len(rows[0]), BLOCK), resync_after=2)
    assert any(e[0] == 4 for ev in evs for e in ev)


def test_nan_fault_leaves_the_stream_untouched(sdr, gpu_ctx):
    """NaN at sample 3 of stream 1's first call: its fault bit, no events, the host layer raises
    on the same row; streams 0 and 2 exact; from the next call on stream 1 equals a host layer
    that made the failed call and then the clean ones."""
    bad = _row(7).copy()
    bad[3] = np.nan
    rows = [_row(5), bad, _row(9)]
    cuts = _cuts(len(bad), BLOCK)
    dev = _device(sdr, gpu_ctx, rows, cuts)
    host = [_host(sdr, x, cuts) for x in rows]
    assert host[1][0] is None and all(r is not None for r in host[1][1:])
    ev, status, counts, bd = dev[0]
    assert status[1] & sdr.RdsLinkBank.FAULT and ev[1] == [] and counts[1] == 0
    assert len(bd[1][0]) == 0 and len(bd[1][1]) == 0
    assert status[0] == 0 and status[2] == 0
    _check_stream(dev, host[0], 0)
    _check_stream(dev, host[2], 2)
    _check_stream(dev[1:], host[1][1:], 1)
    # a last symbol that is NaN, in a later call: the same rule
    late = _row(5).copy()
    host0 = _host(sdr, late, cuts)
    ns = len(host0[1]["symbols"])
    off = int(np.flatnonzero(late[BLOCK:2 * BLOCK] == np.float32(host0[1]["symbols"][-1]))[-1])
    assert off >= BLOCK - 24 and ns >= 2
    late[BLOCK + off] = np.nan
    host1 = _host(sdr, late, cuts)
    assert host1[1] is None and all(r is not None for k, r in enumerate(host1) if k != 1)
    dev = _device(sdr, gpu_ctx, [late, _row(9)], cuts)
    assert dev[1][1][0] & sdr.RdsLinkBank.FAULT and dev[1][0][0] == []
    _check_stream(dev[:1] + dev[2:], host1[:1] + host1[2:], 0)
    _check_stream(dev, host[2], 1)


def test_event_overflow(sdr, gpu_ctx):
    """max_events=2: the true counts are reported, the overflow bit is set, and the next call's
    events still equal the host's."""
    x = _row(5)
    cuts = [4 * BLOCK, 2 * BLOCK, 2 * BLOCK]
    host = _host(sdr, x, cuts)
    dev = _device(sdr, gpu_ctx, [x], cuts, max_events=2)
    over = 0
    for (ev, status, counts, bd), ref in zip(dev, host):
        assert counts[0] == len(ref["events"])
        assert [e[:3] for e in ev[0]] == ref["events"][:2]
        assert bool(status[0] & sdr.RdsLinkBank.OVERFLOW) == (len(ref["events"]) > 2)
        over += len(ref["events"]) > 2
        np.testing.assert_array_equal(bd[0][1], ref["diff"])
    assert over >= 2 and len(host[2]["events"]) >= 1


def test_arguments(sdr, gpu_ctx):
    bank = sdr.RdsLinkBank(2, 4000, ctx=gpu_ctx)
    buf = sdr.DeviceBuffer(gpu_ctx, 2 * 4040 * 4)
    buf.zero()
    for n, stride in ((1535, 4040), (4001, 4040), (4000, 3999), (2000, 1999)):
        with pytest.raises(ValueError):
            bank.process_dev(buf.ptr, n, stride)
    with pytest.raises(ValueError):
        bank.process_dev(0, 2000, 2000)
    with pytest.raises(ValueError):
        bank.bits(2)
    bank.process_dev(buf.ptr, 4000, 4040)            # the limits themselves are legal
    bank.process_dev(buf.ptr, 1536, 1536)
    bank.close()
    buf.free()
    for bad in (dict(nstreams=0, max_n=4000), dict(nstreams=1, max_n=1535), dict(nstreams=1, max_n=4000, max_events=0)):
        with pytest.raises(ValueError):
            sdr.RdsLinkBank(ctx=gpu_ctx, **bad)
    rx = sdr.Receiver(1, 51_200, mono=True, ctx=gpu_ctx)
    with pytest.raises(ValueError):
        rx.rds_link()
    rx.close()


def test_receiver_end_to_end(sdr, gpu_ctx, golden):
    """Three u8 streams through Receiver.process_dev + RdsLinkBank.process_rx: stream 0 is the
    golden file's IQ and gives the reference script's prints; every stream equals the host layer
    on the fetched rrc_i rows."""
    z = golden("rds_link.npz")
    nblk, B = len(z["rrc_i"]), 153_600
    assert int(z["n_complex"]) >= nblk * B
    iq = [sdr.synth.fm_iq(nblk * B, seed=sd, dtype=np.uint8, rds_groups=True)
          for sd in (int(z["seed"]), int(z["seed"]) + 1, int(z["seed"]) + 2)]
    iq[0] = sdr.synth.fm_iq(int(z["n_complex"]), seed=int(z["seed"]), dtype=np.uint8, rds_groups=True)[:2 * nblk * B]
    rx = sdr.Receiver(3, B, mono=False, rds=True, iq_dtype=np.uint8, ctx=gpu_ctx)
    bank = rx.rds_link()
    links = [sdr.RdsLinkLayer() for _ in range(3)]
    dev, host = [], [[] for _ in range(3)]
    for k in range(nblk):
        blk = np.stack([x[2 * k * B:2 * (k + 1) * B] for x in iq])
        buf = sdr.DeviceBuffer.from_array(gpu_ctx, blk)
        rx.process_dev(buf.ptr, B)
        bank.process_rx(rx)
        ev, status = bank.events()
        dev.append((ev, status, bank.counts.copy(), [bank.bits(s) for s in range(3)]))
        rrc = rx.output("rrc_i")
        for s in range(3):
            host[s].append(links[s].process(rrc[s]))
        buf.free()
    events = [_check_stream(dev, host[s], s) for s in range(3)]
    assert [e[:3] for e in events[0]] == [tuple(int(v) for v in e) for e in z["events"]]
    bank.close()
    rx.close()


def test_reset_reproduces_the_first_pass(sdr, gpu_ctx):
    rows = [_row(5), _half(_row(7))[24:]]
    total = min(len(x) for x in rows)
    cuts = _cuts(total, BLOCK)
    bank = sdr.RdsLinkBank(2, BLOCK, resync_after=2, ctx=gpu_ctx)
    first = _device(sdr, gpu_ctx, rows, cuts, bank=bank)
    bank.reset()
    second = _device(sdr, gpu_ctx, rows, cuts, bank=bank)
    bank.close()
    for s, x in enumerate(rows):
        _check_stream(first, _host(sdr, x, cuts, 2), s)
    for a, b in zip(first, second):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        for (ba, da), (bb, db) in zip(a[3], b[3]):
            np.testing.assert_array_equal(ba, bb)
            np.testing.assert_array_equal(da, db)
