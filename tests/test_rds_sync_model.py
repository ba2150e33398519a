"""The block-sync specification (rtsdr.RdsBlockSync) and the group decoder (rtsdr.RdsProgramme),
pure Python, on the CPU.

Expected values are written down here from the streams' construction (tests/rds_sync_streams.py:
where a block starts, which bits were flipped, which words went in) or come from the committed
link-layer fixture -- never from a second run of the model, except for split invariance, where
one call is compared with many.
"""
import numpy as np
import pytest

import rds_sync_streams as rs

A, B, C, D, CP = range(5)


def _run(sdr, bits, **kw):
    m = sdr.RdsBlockSync(**kw)
    return m.process(bits), m


def test_offset_syndromes(sdr):
    from rtsdr import rdssync
    want = {"A": 0x3D8, "B": 0x3D4, "C": 0x25C, "D": 0x258, "C'": 0x3CC}
    assert rdssync.SYNDROMES == want
    for name, syn in want.items():
        for info in (0, 0xFFFF, 0x1234):
            w = int("".join(str(b) for b in sdr.synth.rds_block_bits(info, name)), 2)
            assert rdssync.syndrome(w) == syn, name


def test_burst_tables(sdr):
    from rtsdr import rdssync
    sizes = []
    for b in range(6):
        t = rdssync.burst_table(b)
        sizes.append(len(t))
        assert 0 not in t
        pats = list(t.values())
        assert len(set(pats)) == len(pats)                      # distinct patterns under distinct syndromes
        for s, pat in t.items():
            assert rdssync.syndrome(pat) == s
            hi, lo = pat.bit_length() - 1, (pat & -pat).bit_length() - 1
            assert 0 < pat < 1 << 26 and hi - lo <= b - 1
    assert sizes == [0, 26, 51, 99, 191, 367]
    for bad in (-1, 6):
        with pytest.raises(ValueError):
            sdr.RdsBlockSync(max_burst=bad)
    for bad in (0, 256):
        with pytest.raises(ValueError):
            sdr.RdsBlockSync(lose_after=bad)


def _fixture_bits(z):
    rows = np.split(z["diff"], np.cumsum(z["n_diff"])[:-1])
    calls = [rows[0]] + [r[27:] for r in rows[1:]]
    assert sum(len(c) for c in calls) == 531
    return calls


@pytest.mark.parametrize("max_burst", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("one_call", [False, True])
def test_golden_fixture(sdr, golden, max_burst, one_call):
    """The link-layer fixture's 531 bits: every third block has the link layer's single flipped
    bit; 20 blocks at 1 + 26 k, all the generator's words once correction is on."""
    z = golden("rds_link.npz")
    calls = _fixture_bits(z)
    if one_call:
        calls = [np.concatenate(calls)]
    m = sdr.RdsBlockSync(max_burst=max_burst)
    rec = [r for c in calls for r in m.process(c)]
    bad = 1 if max_burst else 2
    assert [r[1] for r in rec] == [1 + 26 * k for k in range(20)]
    assert [r[2] for r in rec] == [0, 0, bad] * 6 + [0, 0]
    assert [r[0] for r in rec] == [A, B, C, D] * 5
    rng = np.random.default_rng(int(z["seed"]))
    gen = [int(rng.integers(0, 1 << 16)) for _ in range(20)]
    got = [r[3] for r in rec]
    if max_burst:
        assert got == gen
    else:
        assert [g for g, r in zip(got, rec) if r[2] == 0] == [w for w, r in zip(gen, rec) if r[2] == 0]
    n_bad = 6
    assert m.state() == (1, 1 + 26 * 20, 14, n_bad if max_burst else 0, 0 if max_burst else n_bad, 1, 0)


@pytest.mark.parametrize("junk", [0, 1, 25, 26, 27])
def test_leading_junk(sdr, junk):
    g = rs.groups(3, 4)
    rec, m = _run(sdr, rs.coded(sdr, g, junk, seed=junk))
    assert rec == [(k & 3, junk + 26 * k, 0, w) for k, w in enumerate(rs.words(g))]
    assert m.state() == (1, junk + 26 * 16, 16, 0, 0, 1, 0)


def test_corrections(sdr):
    """Every single-bit error and bursts of 2 .. 5 at both ends and in the middle of block 6 (a C)
    and of block 9 (a B) are corrected with max_burst = 5; each pattern is corrected exactly from
    the max_burst that covers its length on."""
    g = rs.groups(4, 4)
    clean = rs.coded(sdr, g, 3)
    w = rs.words(g)
    cases = rs.correction_cases()
    assert len(cases) == 26 + 3 + 6 + 9 + 9 and max(max(c) for c in cases) == 25
    for offs in cases:
        for blk in (6, 9):
            want = [(k & 3, 3 + 26 * k, int(k == blk), x) for k, x in enumerate(w)]
            rec, m = _run(sdr, rs.flip(clean, blk, offs, 3), max_burst=5)
            assert rec == want, (offs, blk)
            span = offs[-1] - offs[0] + 1
            for b in range(0, 5):
                rec, _ = _run(sdr, rs.flip(clean, blk, offs, 3), max_burst=b)
                assert rec[blk][2] == (1 if b >= span else 2), (offs, b)
                if b >= span:
                    assert rec == want


def test_burst_of_three_needs_max_burst_three(sdr):
    g = rs.groups(5, 3)
    clean = rs.coded(sdr, g)
    w = rs.words(g)
    for offs in ([4, 6], [4, 5, 6], [23, 24, 25]):
        bits = rs.flip(clean, 5, offs)
        rec, m = _run(sdr, bits, max_burst=2)
        received = int("".join(str(b) for b in bits[26 * 5:26 * 5 + 16]), 2)
        assert rec[5] == (B, 26 * 5, 2, received), offs
        assert m.state()[2:5] == (11, 0, 1)
        rec, _ = _run(sdr, bits, max_burst=3)
        assert rec[5] == (B, 26 * 5, 1, w[5])


def test_version_b_groups(sdr):
    g = rs.groups(6, 4, version_b=True)
    clean = rs.coded(sdr, g, 2)
    w = rs.words(g)
    types = [A, B, CP, D] * 4
    rec, _ = _run(sdr, clean)
    assert rec == [(types[k], 2 + 26 * k, 0, x) for k, x in enumerate(w)]
    # a damaged C' is corrected as C' through the B word's version bit (also a corrected B's)
    for b_offs in ([], [7]):
        bits = rs.flip(rs.flip(clean, 6, [20], 2), 5, b_offs, 2)
        rec, _ = _run(sdr, bits)
        assert rec[6] == (CP, 2 + 26 * 6, 1, w[6])
        assert rec[5] == (B, 2 + 26 * 5, int(bool(b_offs)), w[5])
    # ... and not when the B block is uncorrectable: type C, status 2, the bits as received
    bits = rs.flip(rs.flip(clean, 6, [20], 2), 5, rs.UNCORRECTABLE, 2)
    rec, _ = _run(sdr, bits)
    assert rec[5][2] == 2
    received = int("".join(str(b) for b in bits[2 + 26 * 6:2 + 26 * 6 + 16]), 2)
    assert rec[6] == (C, 2 + 26 * 6, 2, received)
    # an undamaged C' after an uncorrectable B is still a C'
    rec, _ = _run(sdr, rs.flip(clean, 5, rs.UNCORRECTABLE, 2))
    assert rec[6] == (CP, 2 + 26 * 6, 0, w[6])
    # a version-A group's damaged C is corrected as C
    ga = rs.groups(6, 4, version_b=False)
    rec, _ = _run(sdr, rs.flip(rs.coded(sdr, ga, 2), 6, [20], 2))
    assert rec[6] == (C, 2 + 26 * 6, 1, rs.words(ga)[6])


def test_flywheel(sdr):
    g = rs.groups(7, 8)
    clean = rs.coded(sdr, g, 5)
    w = rs.words(g)
    # 11 bad blocks and then a good one keep sync
    rec, m = _run(sdr, rs.bad_run(clean, 4, 11, 5))
    assert [r[2] for r in rec] == [0] * 4 + [2] * 11 + [0] * 17
    assert [r[1] for r in rec] == [5 + 26 * k for k in range(32)]
    assert m.state() == (1, 5 + 26 * 32, 21, 0, 11, 1, 0)
    # 12 lose it: the twelfth bad block is still reported, then the next pair acquires again
    rec, m = _run(sdr, rs.bad_run(clean, 4, 12, 5))
    assert [r[2] for r in rec] == [0] * 4 + [2] * 12 + [0] * 16
    assert [r[1] for r in rec] == [5 + 26 * k for k in range(32)]
    assert [r[3] for r in rec[16:]] == w[16:]
    assert m.state() == (1, 5 + 26 * 32, 20, 0, 12, 2, 1)
    # ... and with nothing behind the twelfth the stream ends in SEARCH behind it
    rec, m = _run(sdr, rs.bad_run(clean, 4, 12, 5)[:5 + 26 * 16 + 20])
    assert m.state() == (0, 5 + 26 * 16, 4, 0, 12, 1, 1)
    # corrected blocks do not feed the flywheel: 12 of them in a row lose sync too
    bits = clean
    for k in range(12):
        bits = rs.flip(bits, 4 + k, [9], 5)
    rec, m = _run(sdr, bits)
    assert [r[2] for r in rec] == [0] * 4 + [1] * 12 + [0] * 16 and [r[3] for r in rec] == w
    assert m.state()[5:] == (2, 1)
    # lose_after = 3
    rec, m = _run(sdr, rs.bad_run(clean, 4, 3, 5), lose_after=3)
    assert m.state() == (1, 5 + 26 * 32, 29, 0, 3, 2, 1)


def test_slip(sdr):
    """Seven extra bits before block 8: twelve blocks at the old phase fail, sync is lost, and the
    stream is acquired again at the new phase with the generator's words."""
    g = rs.groups(8, 10)
    w = rs.words(g)
    bits = rs.slipped(rs.coded(sdr, g, 4), 4 + 26 * 8)
    rec, m = _run(sdr, bits)
    pos = [r[1] for r in rec]
    assert all(b > a for a, b in zip(pos, pos[1:]))
    assert rec[:8] == [(k & 3, 4 + 26 * k, 0, w[k]) for k in range(8)]
    assert [r[1] for r in rec[8:20]] == [4 + 26 * k for k in range(8, 20)]
    assert all(r[2] != 0 for r in rec[8:20])
    # the loss is behind old-phase block 19, which ends inside new-phase block 19: from block 20 on
    first = 20
    assert rec[20:] == [(k & 3, 11 + 26 * k, 0, w[k]) for k in range(first, 40)]
    assert m.state()[0] == 1 and m.state()[5:] == (2, 1)


@pytest.mark.parametrize("size", [1, 25, 26, 27, 51, 52])
def test_split_invariance(sdr, size):
    streams = [rs.slipped(rs.bad_run(rs.coded(sdr, rs.groups(9, 12, None), 30), 6, 12, 30), 30 + 26 * 30),
               rs.noisy(sdr, 13, 3000, 0.05)]
    for bits in streams:
        whole, m = _run(sdr, bits)
        assert m.acquisitions >= 2 and m.losses >= 1
        for cuts in (rs.cuts_of(len(bits), size), rs.random_cuts(len(bits), size)):
            calls = rs.model_calls(sdr, bits, cuts)
            assert [r for rec, _ in calls for r in rec] == whole
            assert calls[-1][1] == m.state()
    assert sdr.RdsBlockSync().process([]) == []


def _programme(sdr, grps, damage=()):
    bits = sdr.synth.rds_group_bits(grps)
    for blk in damage:
        bits = rs.flip(bits, blk, rs.UNCORRECTABLE)
    m, p = sdr.RdsBlockSync(), sdr.RdsProgramme()
    rec = m.process(bits)
    p.feed(rec[:7])                 # in two feeds: a group may straddle them
    p.feed(rec[7:])
    return p, rec


def test_programme_ps_and_radiotext(sdr):
    syn = sdr.synth
    grps = syn.rds_ps_groups(0x54A8, "HIP FM 1", pty=10, tp=1) + syn.rds_rt_groups(0x54A8, "Now playing: gfx950 ~ {x}\x7f\x01", pty=10, tp=1)
    p, rec = _programme(sdr, grps)
    assert len(rec) == 4 * len(grps) and p.groups == len(grps)
    assert (p.pi, p.pty, p.tp) == (0x54A8, 10, 1)
    assert p.ps == "HIP FM 1" and p.ps_complete
    assert p.radiotext == "Now playing: gfx950 ~ {x}??"
    # a full 64-character text has no end mark; a flag change clears the old text
    long_text = "".join(chr(0x21 + k) for k in range(64))
    p, _ = _programme(sdr, syn.rds_rt_groups(1, long_text) + syn.rds_rt_groups(1, "short", flag=1))
    assert p.radiotext == "short"
    p, _ = _programme(sdr, syn.rds_rt_groups(1, long_text))
    assert p.radiotext == long_text
    p, _ = _programme(sdr, syn.rds_rt_groups(1, long_text) + syn.rds_rt_groups(1, "short"))
    assert p.radiotext == "short"                                  # same flag: overwritten, 0x0D ends it
    p, _ = _programme(sdr, syn.rds_rt_groups(1, long_text) + syn.rds_rt_groups(1, "ab", flag=1, version_b=True))
    assert p.radiotext == "ab"


def test_programme_missing_segment_until_repeated(sdr):
    syn = sdr.synth
    once = syn.rds_ps_groups(0x1001, "ABCDEFGH")
    p, rec = _programme(sdr, once + once[:1], damage=[4 * 2 + 3])   # segment 2's D block
    assert rec[11][2] == 2
    assert p.ps == "ABCD  GH" and not p.ps_complete and p.groups == 4
    p, _ = _programme(sdr, once + once, damage=[4 * 2 + 3])
    assert p.ps == "ABCDEFGH" and p.ps_complete
    # a damaged A block loses the group too, and a corrected block does not
    p, _ = _programme(sdr, once + once[:1], damage=[4])
    assert p.ps == "AB  EFGH" and not p.ps_complete
    bits = rs.flip(syn.rds_group_bits(once), 7, [3])
    p = sdr.RdsProgramme()
    p.feed(sdr.RdsBlockSync().process(bits))
    assert p.ps == "ABCDEFGH" and p.ps_complete


def test_programme_version_b_and_pi_change(sdr):
    syn = sdr.synth
    grps = syn.rds_ps_groups(0x2002, "B-GROUPS", version_b=True, pty=3)
    p, rec = _programme(sdr, grps)
    assert [r[0] for r in rec[:4]] == [A, B, CP, D]
    assert (p.pi, p.pty, p.ps, p.ps_complete) == (0x2002, 3, "B-GROUPS", True)
    # PI is taken from block C' of a version-B group
    odd = [(0x7777, b, c, d) for _, b, c, d in grps[:1]]
    p, _ = _programme(sdr, odd)
    assert p.pi == 0x2002
    # a new PI starts the name again
    p, _ = _programme(sdr, syn.rds_ps_groups(0x1111, "OLDNAME ") + syn.rds_ps_groups(0x2222, "NEW")[:2])
    assert p.pi == 0x2222 and p.ps == "NEW     "[:4] + "    " and not p.ps_complete
