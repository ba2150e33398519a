"""The block receiver's allocation layout (csrc/rx_layout.h) on the CPU: the header is plain C++,
so a stand-alone program (tests/rx_layout_main.cpp) built with the host compiler and the address
and undefined-behaviour sanitizers prints it for a grid of geometries, and the output is held
against the rule rx_finalize applied by hand before the header existed, restated here in Python
integers without reading the header:

  * f32 rows: per row set, the outputs the flags produce in enum order, S rows each; n = M, M + 1,
    A or R by length class; stride round_up(n, 64) -- except that the M-long rows share the
    (M + 1)-long rows' stride round_up(M + 1, 64) --; a 64-float gap after every output;
  * f64 regions from the next 64-B boundary: two state banks (per used state slot
    round_up(max(T_f - 1, 1) * S, 2) doubles, T_f its filter's tap count), then phase, wraps, last_phi (S2 = round_up(S, 2)
    doubles each), two PLL states (6 S2), theta and pllc rows for every row set;
  * pllw at the next 256-B boundary (per row set round_up(pllw_bytes, 256)), then the sign codes;
  * total = the sizes + 64 + 256: each alignment is budgeted whole.
"""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUDIO, STEREO, RDS = 1, 2, 4
GRID = list(itertools.product([1, 3, 8], [1, 10, 1000, 51200, 614400], [0, AUDIO, STEREO, RDS, STEREO | RDS],
                              [0, 1], [1, 2, 3], [1, 101, 151], [0, 4352]))
# per SDR_RX_O_*: (group, needs de-emphasis, length class); per SDR_RX_F_*: its group; per Z_*: its filter, which has
# T + (its index) taps, so that a state slot tied to the wrong filter shows in zlen and zoff
ALWAYS, G_AU, G_ST, G_RD = range(4)
OUTPUTS = ([(ALWAYS, 0, "M"), (G_AU, 0, "A"), (G_ST, 0, "M"), (G_ST, 0, "M1"), (G_ST, 0, "M")] + [(G_ST, 0, "A")] * 3 +
           [(G_RD, 0, "M")] * 2 + [(G_RD, 0, "M1")] * 2 + [(G_RD, 0, "M")] * 2 + [(G_RD, 0, "R")] * 4 +
           [(G_AU, 1, "A"), (G_ST, 1, "A"), (G_ST, 1, "A")])
FILTERS = [ALWAYS, G_AU, G_ST, G_ST, G_ST] + [G_RD] * 5
STATES = [0, 0, 1, 2, 3, 5, 6, 4, 7, 7, 8, 8, 9, 9]


def up(v, m):
    return (v + m - 1) // m * m


def on(flags, group):
    return [True, bool(flags & (AUDIO | STEREO)), bool(flags & STEREO), bool(flags & RDS)][group]


def parent_rule(S, B, flags, de, nsets, T, pllw):
    """What rx_finalize computed before rx_layout.h: byte offsets from the allocation's base."""
    M = -(-B // 10)
    A, R = -(-M // 5), -(-M * 19 // 80)
    n_of = {"M": M, "M1": M + 1, "A": A, "R": R}
    st_of = {"M": up(M + 1, 64), "M1": up(M + 1, 64), "A": up(A, 64), "R": up(R, 64)}
    need = [on(flags, g) and (not d or de) for g, d, _ in OUTPUTS]
    out_n = [n_of[c] if k else 0 for k, (_, _, c) in zip(need, OUTPUTS)]
    out_stride = [st_of[c] if k else 0 for k, (_, _, c) in zip(need, OUTPUTS)]
    floats, out = 0, [[(-1, 0)] * len(OUTPUTS) for _ in range(3)]
    for q in range(nsets):
        for o in range(len(OUTPUTS)):
            if need[o]:
                out[q][o] = (4 * floats, 4 * (out_stride[o] * S + 64))
                floats += out_stride[o] * S + 64
    zl, zoff, zlen = 0, [0] * len(STATES), [0] * len(STATES)
    for z, f in enumerate(STATES):
        if on(flags, FILTERS[f]):
            zoff[z], zlen[z] = zl, max(T + f - 1, 1)
            zl += up(zlen[z] * S, 2)
    ths, cst, pcs, S2 = up(M, 2) + 2, up(M + M // 32, 2) + 2, up(M + 16, 256), up(S, 2)
    doubles = 2 * zl + 3 * S2 + 2 * 6 * S2 + nsets * (2 * S * ths + 2 * S * cst)
    pw = up(pllw, 256)
    code = nsets * 2 * S * pcs if flags & (STEREO | RDS) else 0
    total = floats * 4 + 64 + doubles * 8 + 256 + nsets * pw + code
    d = up(floats * 4, 64)
    phase = d + 16 * zl
    ps0 = phase + 24 * S2
    theta = ps0 + 96 * S2
    pllc = theta + 8 * nsets * 2 * S * ths
    pllw_off = up(pllc + 8 * nsets * 2 * S * cst, 256)
    reg = [(d, 8 * zl), (d + 8 * zl, 8 * zl), (phase, 8 * S2), (phase + 8 * S2, 8 * S2), (phase + 16 * S2, 8 * S2),
           (ps0, 48 * S2), (ps0 + 48 * S2, 48 * S2), (theta, pllc - theta), (pllc, 8 * nsets * 2 * S * cst),
           (pllw_off, nsets * pw), (pllw_off + nsets * pw, code) if code else (-1, 0)]
    pstride, sb = up(2 * A, 64), 8 * (3 * S2 + 2)
    pb = 2 * S * pstride
    if de:
        reg += [(0, 16 * S2), (16 * S2, 8 * (S2 + 2))]
        pcm = [(sb + q * pb, pb) if q < nsets else (-1, 0) for q in range(3)]
    else:
        reg += [(-1, 0), (-1, 0)]
        pcm, pstride = [(-1, 0)] * 3, 0
    flat = lambda pairs: [v for p in pairs for v in p]
    return {"sizes": [M, A, R, zl, ths, cst, pcs, pw, pstride, total, sb + nsets * pb if de else 0],
            "out_n": out_n, "out_stride": out_stride, "zoff": zoff, "zlen": zlen, "out": [flat(row) for row in out],
            "reg": flat(reg), "pcm": flat(pcm), "reset": [d, 8 * (2 * zl + 2 * S2)], "de_reset": [0, 24 * S2] if de else [-1, 0]}


REG = ["bank0", "bank1", "phase", "wraps", "last_phi", "pll_state0", "pll_state1", "theta", "pllc", "pllw", "pcode",
       "de_state", "de_mono"]


def pairs(flat):
    return list(zip(flat[0::2], flat[1::2]))


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler (g++, c++, clang++) on PATH: rx_layout.h is not checked")
    exe = tmp_path_factory.mktemp("rx_layout") / "rx_layout_main"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "rx_layout_main.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)] + [str(v) for g in GRID for v in g], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    got, cur = {}, None
    for line in r.stdout.splitlines():
        key, *vals = line.split()
        if key == "geom":
            cur = got[tuple(int(v) for v in vals)] = {"out": []}
        elif key == "out":
            cur["out"].append([int(v) for v in vals])
        elif key != "end":
            cur[key] = [int(v) for v in vals]
    assert sorted(got) == sorted(GRID)
    return got


def test_matches_the_restated_rule(layouts):
    for g in GRID:
        want, got = parent_rule(*g), layouts[g]
        for key, val in want.items():
            assert got[key] == val, (g, key)


def test_regions_inside_and_disjoint(layouts):
    for g in GRID:
        L = layouts[g]
        reg = dict(zip(REG, pairs(L["reg"])))
        main = [r for row in L["out"] for r in pairs(row)] + [reg[k] for k in REG[:11]]
        de = [reg["de_state"], reg["de_mono"]] + pairs(L["pcm"])
        for total, regs in ((L["sizes"][9], main), (L["sizes"][10], de)):
            end = 0
            for off, size in sorted(r for r in regs if r[0] >= 0):
                assert off >= end and size >= 0 and off + size <= total, (g, off, size)
                end = off + size
        assert all(size == 0 for off, size in main + de if off < 0), g


def test_alignment(layouts):
    for g in GRID:
        L = layouts[g]
        S, reg = g[0], dict(zip(REG, pairs(L["reg"])))
        assert all(off % 16 == 0 for row in L["out"] for off, _ in pairs(row) if off >= 0), g   # f32 rows: 16-B vector accesses
        assert all(s % 4 == 0 for s in L["out_stride"]), g
        ths, cst, pw = L["sizes"][4], L["sizes"][5], L["sizes"][7]
        assert reg["theta"][0] % 16 == 0 and reg["pllc"][0] % 16 == 0 and (8 * ths) % 16 == 0 and (8 * cst) % 16 == 0, g
        assert all(reg[k][0] % 8 == 0 for k in ("bank0", "bank1", "phase", "pll_state0", "pll_state1")), g
        assert reg["wraps"][0] % 4 == 0 and reg["last_phi"][0] % 4 == 0, g
        assert reg["pllw"][0] % 256 == 0 and pw % 256 == 0, g                            # base: 256-B aligned (hipMalloc)
        assert reg["phase"][1] >= 8 * S and reg["wraps"][1] >= 4 * S and reg["last_phi"][1] >= 4 * S, g


def test_reset_range(layouts):
    for g in GRID:
        L = layouts[g]
        reg = dict(zip(REG, pairs(L["reg"])))
        lo, size = L["reset"]
        for k in ("bank0", "bank1", "phase", "wraps"):
            assert lo <= reg[k][0] and sum(reg[k]) <= lo + size, (g, k)
        assert all(reg[k][0] >= lo + size for k in ("last_phi", "pll_state0", "pll_state1")), g
