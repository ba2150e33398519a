"""The split of a range into head elements, 16-B vectors and tail elements (csrc/sdr_range.h) on the
CPU: the header is plain C++, so a stand-alone program (tests/pass_range_main.cpp) built with the
host compiler and the address and undefined-behaviour sanitizers prints the split of every element
size, start and length, reading each range as a pass does from a heap block that ends with it.  The
device passes (iqc.hip, ingest.hip, rmeter.hip through sdr_chunk.h) take their ranges apart with the
same function: this is where "no access leaves the range" is pinned."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def splits(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler (g++, c++, clang++) on PATH: sdr_range.h is not checked")
    exe = tmp_path_factory.mktemp("pass_range") / "pass_range_main"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "pass_range_main.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    got = {}
    for line in r.stdout.splitlines():
        key, *vals = line.split()
        assert key == "range"
        es, start, length, head, nv, tail = (int(v) for v in vals)
        got[es, start, length] = (head, nv, tail)
    return got


@pytest.mark.parametrize("es", (2, 4, 8))
def test_split_covers_the_range_and_nothing_else(splits, es):
    per = 16 // es
    cases = [(start, length) for start in range(0, 16, es) for length in range(3 * per + 4)]
    assert sorted(k[1:] for k in splits if k[0] == es) == cases
    for start, length in cases:
        head, nv, tail = splits[es, start, length]
        assert head + nv * per + tail == length, (start, length)
        assert 0 <= head < per and 0 <= tail < per and nv >= 0, (start, length)
        if nv:
            assert (start + head * es) % 16 == 0, (start, length)
        # the bytes touched: [start, start + head es), the vectors, the tail -- contiguous, so the last
        # byte touched is the range's last byte
        end = start + head * es + 16 * nv + tail * es
        assert end == start + length * es, (start, length)
        first = 16 if start else 0                              # every vector that fits is taken as one
        assert nv == max(0, (start + length * es - first) // 16), (start, length)
