"""Hand-built RDS bit streams for the block-sync tests (tests/test_rds_sync_model.py on the CPU,
tests/test_rds_sync.py on the GPU): coded groups from synth.rds_block_bits with junk prefixes,
error patterns at chosen places, version-B groups, bad runs, a slip and seeded bit errors."""
import numpy as np

UNCORRECTABLE = (0, 13)        # flipped bits of a block that no burst of <= 5 explains


def groups(seed, count, version_b=False):
    """`count` groups of random words; version_b sets (True) or clears (False) every B word's
    version bit, None leaves it random."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        a, b, c, d = (int(rng.integers(0, 1 << 16)) for _ in range(4))
        if version_b is not None:
            b = (b | 0x800) if version_b else (b & ~0x800)
        out.append((a, b, c, d))
    return out


def words(grps):
    return [w for g in grps for w in g]


def coded(sdr, grps, junk=0, seed=0):
    """`junk` seeded random bits, then the groups' 104 bits each"""
    pre = np.random.default_rng(1000 + seed).integers(0, 2, junk).tolist()
    return [int(b) for b in pre] + sdr.synth.rds_group_bits(grps)


def flip(bits, block, offsets, junk=0):
    """the stream with the given bit offsets of block number `block` (0 = the first A) flipped"""
    out = list(bits)
    for o in offsets:
        out[junk + 26 * block + o] ^= 1
    return out


def burst(length, fill):
    """the offsets of a burst of `length` from 0: both ends flipped, the inner bits as the bits of `fill`"""
    if length == 1:
        return [0]
    return [0] + [1 + k for k in range(length - 2) if (fill >> k) & 1] + [length - 1]


def correction_cases():
    """(first bit, offsets relative to the block) of every single-bit error and of bursts of 2 .. 5
    at both ends and in the middle of a block, each with its inner bits all clear, all set and
    alternating"""
    cases = [[e] for e in range(26)]
    for length in range(2, 6):
        for first in (0, 10, 26 - length):
            for fill in {0, (1 << (length - 2)) - 1, 0b101 & ((1 << max(length - 2, 0)) - 1)}:
                cases.append([first + o for o in burst(length, fill)])
    return cases


def bad_run(bits, first_block, count, junk=0):
    """`count` blocks from `first_block` on made uncorrectable"""
    for k in range(count):
        bits = flip(bits, first_block + k, UNCORRECTABLE, junk)
    return bits


def slipped(bits, at, extra=7):
    """`extra` zero bits inserted before bit `at`"""
    return bits[:at] + [0] * extra + bits[at:]


def noisy(sdr, seed, nbits, ber):
    """coded groups with seeded independent bit errors at rate `ber`"""
    bits = np.array(coded(sdr, groups(seed, nbits // 104 + 1, None))[:nbits], dtype=np.uint8)
    err = np.random.default_rng(seed + 500).random(nbits) < ber
    return (bits ^ err).astype(np.uint8).tolist()


def cuts_of(total, size):
    """calls of `size` bits and the rest"""
    out = [size] * (total // size)
    if total % size:
        out.append(total % size)
    return out


def random_cuts(total, seed, top=300, empty=0.2):
    """random call sizes 0 .. top, some of them empty, that add up to `total`"""
    rng = np.random.default_rng(seed)
    out, left = [], total
    while left:
        n = 0 if rng.random() < empty else int(min(left, rng.integers(1, top + 1)))
        out.append(n)
        left -= n
    return out


def model_calls(sdr, bits, cuts, **kw):
    """the model over the cuts of one stream: per call (records, state)"""
    m = sdr.RdsBlockSync(**kw)
    out, o = [], 0
    for n in cuts:
        rec = m.process(bits[o:o + n])
        out.append((rec, m.state()))
        o += n
    return out
