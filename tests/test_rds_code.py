"""The RDS (26, 16) code as the C++ side has it (csrc/rds_code.h) against the specification
(rtsdr.rdssync) on the CPU: the header's host half is plain C++, so a stand-alone program
(tests/rds_code_main.cpp) built with the host compiler and the address and undefined-behaviour
sanitizers prints the syndrome of every one-bit pattern, the offset words and the burst table for
every max_burst, and the output is held against rdssync.syndrome, SYNDROMES and burst_table.  The
device kernels and the host link layer take their parity matrix from the same header."""
import os
import shutil
import subprocess

import pytest

from rtsdr import rdssync

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = {0: 0, 1: 26, 2: 51, 3: 99, 4: 191, 5: 367}


@pytest.fixture(scope="module")
def code(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler (g++, c++, clang++) on PATH: rds_code.h is not checked")
    exe = tmp_path_factory.mktemp("rds_code") / "rds_code_main"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "rds_code_main.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    got = {"bit": {}, "offset": {}, "table": {}}
    for line in r.stdout.splitlines():
        key, *vals = line.split()
        vals = [int(v) for v in vals]
        if key == "none":
            got["none"] = vals[0]
        elif key == "table":
            got["table"][vals[0]] = (vals[1], vals[2], dict(zip(vals[3::2], vals[4::2])))
        else:
            got[key][vals[0]] = tuple(vals[1:])
    return got


def test_one_bit_syndromes_are_the_rows_of_h(code):
    assert sorted(code["bit"]) == list(range(26))
    for j in range(26):
        assert code["bit"][j] == (rdssync.syndrome(1 << (25 - j)),), j
    assert len({s for s, in code["bit"].values()}) == 26


def test_offset_words(code):
    assert sorted(code["offset"]) == list(range(5))
    for t, name in enumerate(rdssync.TYPE_NAMES):
        syn, typ, slot = code["offset"][t]
        assert (syn, typ, slot) == (rdssync.SYNDROMES[name], t, (0, 1, 2, 3, 2)[t]), name
    assert code["none"] == 7                    # no offset word: the value the window entries hold in three bits


@pytest.mark.parametrize("max_burst", sorted(PATTERNS))
def test_burst_table(code, max_burst):
    collided, count, table = code["table"][max_burst]
    want = rdssync.burst_table(max_burst)
    assert collided == 0 and count == len(table) == len(want) == PATTERNS[max_burst]
    assert table == {s: 1 << 16 | pat >> 10 for s, pat in want.items()}
