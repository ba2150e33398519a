"""Synthetic RRC-output rows for the symbol-clock tests (tests/test_rds_clock_model.py on the CPU,
tests/test_rds_clock.py on the GPU): coded groups from synth.rds_group_bits, differentially and
Manchester coded as synth.rds_symbols does, shaped with raised-cosine pulses (beta = 0.9) at
24 (1 + ppm 1e-6) samples per symbol, float32, with seeded white noise."""
import functools

import numpy as np

BETA = 0.9
GROUPS = 40                     # 160 blocks, 4 160 bits, 8 320 symbols, about 200 k samples


def gen_words(seed, groups=GROUPS):
    """the generator's information words, one per block, version-A groups"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(groups):
        a, b, c, d = (int(rng.integers(0, 1 << 16)) for _ in range(4))
        out.append((a, b & ~0x800, c, d))
    return out


def symbols_of(sdr, grps):
    """+-1 biphase symbols of the groups: e_t = e_(t-1) xor d_t, e = 1 -> (+1, -1), e = 0 -> (-1, +1)"""
    bits = sdr.synth.rds_group_bits(grps)
    e = np.bitwise_xor.accumulate(np.array(bits, dtype=np.int64))
    sym = np.empty(2 * len(bits))
    sym[0::2] = np.where(e == 1, 1.0, -1.0)
    sym[1::2] = -sym[0::2]
    return sym


def raised_cosine(t):
    """the raised-cosine pulse at t symbols from its peak"""
    t = np.asarray(t, dtype=np.float64)
    den = 1.0 - (2.0 * BETA * t) ** 2
    safe = np.where(np.abs(den) < 1e-9, 1.0, den)
    v = np.sinc(t) * np.cos(np.pi * BETA * t) / safe
    return np.where(np.abs(den) < 1e-9, np.pi / 4 * np.sinc(1.0 / (2.0 * BETA)), v)


def shape(sym, ppm=0.0, delay=0.0, sigma=0.05, seed=0):
    """the symbols as a float32 row: symbol k peaks at sample delay + 12 + k 24 (1 + ppm 1e-6)"""
    sps = 24.0 * (1.0 + ppm * 1e-6)
    n = int(len(sym) * sps)
    t = (np.arange(n, dtype=np.float64) - delay - 12.0) / sps
    k0 = np.floor(t).astype(np.int64)
    a = np.concatenate([np.zeros(4), sym, np.zeros(5)])
    x = np.zeros(n)
    for q in range(-3, 5):
        x += a[k0 + q + 4] * raised_cosine(t - (k0 + q))
    x += np.random.default_rng(seed + 100).normal(0.0, sigma, n)
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _row(ppm, delay, sigma, seed, insert_at, groups):
    import rtsdr as sdr
    sym = symbols_of(sdr, gen_words(seed, groups))
    if insert_at is not None:
        sym = np.concatenate([sym[:insert_at], [-sym[insert_at - 1]], sym[insert_at:]])
    x = shape(sym, ppm, delay, sigma, seed)
    x.setflags(write=False)
    return x


def row(ppm=0.0, delay=0, sigma=0.05, seed=0, insert_at=None, groups=GROUPS):
    """A read-only float32 row (cached).  insert_at: one extra symbol, the opposite of its
    predecessor, in front of symbol `insert_at`."""
    return _row(float(ppm), float(delay), float(sigma), int(seed), insert_at, int(groups))


def words(seed, groups=GROUPS):
    return [w for g in gen_words(seed, groups) for w in g]


def generator_blocks(records, seed, groups=GROUPS):
    """how many of the generator's blocks are among the records with status <= 1, each once"""
    left = {}
    for w in words(seed, groups):
        left[w] = left.get(w, 0) + 1
    hit = 0
    for _, _, status, word in records:
        if status <= 1 and left.get(int(word), 0) > 0:
            left[int(word)] -= 1
            hit += 1
    return hit


def clock_blocks(sdr, x, seed, groups=GROUPS, **kw):
    """generator blocks through RdsSymbolClock and RdsBlockSync"""
    clk = sdr.RdsSymbolClock(**kw)
    return generator_blocks(sdr.RdsBlockSync().process(clk.process(x)), seed, groups)


def link_blocks(sdr, oracle, x, seed, groups=GROUPS):
    """generator blocks through the existing rule: oracle.rds_link on the whole row as one block,
    its diff bits into RdsBlockSync"""
    diff = oracle.rds_link([np.asarray(x, dtype=np.float64)])[0]["diff"]
    return generator_blocks(sdr.RdsBlockSync().process(diff.astype(np.uint8)), seed, groups)


def random_cuts(total, seed, top=3000, empty=0.15):
    """random call sizes 0 .. top, some of them empty, that add up to `total`"""
    rng = np.random.default_rng(seed)
    out, left = [], total
    while left:
        n = 0 if rng.random() < empty else int(min(left, rng.integers(0, top + 1)))
        out.append(n)
        left -= n
    return out


def model_calls(sdr, x, cuts, **kw):
    """the model over the cuts of one row: per call (bits, state)"""
    m = sdr.RdsSymbolClock(**kw)
    out, o = [], 0
    for n in cuts:
        out.append((m.process(x[o:o + n]), m.state()))
        o += n
    return out
