"""bench.py's options on CPU: what a plain run leaves out and --full puts back, and the
--dump-outputs writer (whole arrays within the budget, a fixed seeded sample beyond it)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_measures_the_headline_only(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.steps, a.warmup, a.workload) == (7, 3, "mono")
    assert not a.full and not a.cpu and not a.extras and a.dump_outputs is None


def test_full_run_keeps_every_leg_and_its_off_switches(monkeypatch):
    a = parse(monkeypatch, "--full")
    assert a.full and a.cpu and a.extras and a.steps == 50
    a = parse(monkeypatch, "--full", "--no-cpu")
    assert a.extras and not a.cpu
    a = parse(monkeypatch, "--full", "--no-extras")
    assert a.cpu and not a.extras


def test_bad_step_counts_and_dump_of_other_workloads_are_refused(monkeypatch):
    for argv in (["--steps", "0"], ["--warmup", "-1"], ["--workload", "c5", "--dump-outputs", "x"]):
        with pytest.raises(SystemExit):
            parse(monkeypatch, *argv)


def test_input_is_the_same_at_any_thread_count(sdr):
    """The headline's input is built by several threads; every sample must be the one a single
    thread makes (runs and builds are compared output for output).  Chunks of 1 000 over 10 500
    samples: full groups of chunks, a short last group and a short last chunk."""
    kw = dict(seed=3, chunk=1000, rds_groups=True, rds_phase=0.3, pilot_offset_hz=1.5, clock_ppm=20.0)
    one = sdr.synth.fm_iq(10_500, **kw)
    assert one.dtype == np.float32 and one.shape == (21_000,) and np.isfinite(one).all()
    for threads in (3, 4, 64):
        assert np.array_equal(sdr.synth.fm_iq(10_500, threads=threads, **kw), one)
    assert np.array_equal(sdr.synth.fm_iq(10_500, threads=5, dtype=np.uint8, **kw),
                          sdr.synth.fm_iq(10_500, dtype=np.uint8, **kw))
    assert bench.synth_threads() >= 1


def test_dump_outputs_whole_within_budget(tmp_path):
    x = np.arange(1000, dtype=np.float32)
    y = np.linspace(-1, 1, 77)                      # f64 in: written as float32
    bench.dump_outputs(str(tmp_path / "d"), {"audio": x, "demod": y})
    got = np.load(tmp_path / "d" / "audio.npy")
    assert got.dtype == np.float32 and np.array_equal(got, x)
    got = np.load(tmp_path / "d" / "demod.npy")
    assert got.dtype == np.float32 and np.array_equal(got, y.astype(np.float32))


def test_dump_outputs_samples_beyond_budget(tmp_path):
    x = np.arange(3000, dtype=np.float32)
    y = -np.arange(1000, dtype=np.float32)
    budget = 4000                                   # bytes: a quarter of the 16 000 there are
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"x": x, "y": y}, budget=budget)
    ax, ay = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "a" / "y.npy")
    assert ax.size == 750 and ay.size == 250 and ax.nbytes + ay.nbytes <= budget
    # elements of the arrays themselves, in order, none twice; the same ones every time
    assert np.all(np.diff(ax) > 0) and np.all(np.diff(ay) < 0)
    assert np.array_equal(ax, np.load(tmp_path / "b" / "x.npy"))
    assert np.array_equal(ay, np.load(tmp_path / "b" / "y.npy"))
