"""The device-side cascade of second-order sections (RowSos, csrc/sos.hip) against scipy.signal.sosfilt
in float64 (tests/test_sos_model.py pins rtsdr.sos_model to it on the CPU).

The bound is tests/sos_rows.py's: |y - y_ref| <= 2^-24 |y_ref| + 16 e_ref + 2^-50 G per sample and
|zf - zf_ref| <= 16 e_ref + 2^-50 G, e_ref the reference's own rounding noise against a long-double
loop, computed on the CPU.  The rows sit between guards of 1e30, which must come back unchanged and
would show in any output they leaked into.  Every test prints the worst share of the bound it saw."""
import ctypes

import numpy as np
import pytest

import sos_rows as sr

pytestmark = pytest.mark.gpu

OFFSETS = ((0, 0), (1, 3), (3, 1))       # floats past a 16-byte boundary: the input rows, the output rows


@pytest.fixture(scope="module")
def refs():
    return sr.references()


@pytest.fixture(scope="module")
def bufs(sdr, gpu_ctx):
    a, b = sr.Rows(sdr, gpu_ctx, sr.S * (sr.NMAX + 16)), sr.Rows(sdr, gpu_ctx, sr.S * (sr.NMAX + 16))
    yield a, b
    a.free()
    b.free()


def run(filt, bufs, x, off=(0, 0), gap=5, y=True):
    """one call on x [rows, n] placed between guards; returns the output rows (None without y) after
    checking that nothing else moved"""
    xin, yout = bufs
    rows, n = x.shape
    xp, xs = xin.place(x, off[0], n + gap)
    if y:
        yp, ys = yout.guards(rows, n, off[1], n + gap + 3)
        filt.process_dev(xp, xs, yp, ys, n)
        out, rest = yout.fetch()
        assert np.all(rest == sr.GUARD), "a store outside the output rows"
    else:
        filt.process_dev(xp, xs, None, 0, n)
        out = None
    got, rest = xin.fetch()
    assert np.array_equal(got.view(np.uint32), x.view(np.uint32)) and np.all(rest == sr.GUARD), "the input moved"
    return out


@pytest.mark.parametrize("name", sr.SETS)
def test_lengths_alignments_and_guards(sdr, gpu_ctx, refs, bufs, name):
    """every length around a lane, a wave, a tile and a carry lane's chain, on 1 and 3 rows, the rows
    0, 1 and 3 floats past a 16-byte boundary, stride > n"""
    ref = refs[name]
    worst_y = worst_z = worst_d = 0.0
    for rows in (1, 3):
        filt = sdr.RowSos(rows, ref.sos, ctx=gpu_ctx)
        sel = slice(0, rows)
        for n in sr.LENGTHS:
            for off in OFFSETS:
                filt.reset()
                y = run(filt, bufs, ref.x[sel, :n], off)
                assert np.all(np.isfinite(y)) and np.max(np.abs(y)) < 1e6, (name, rows, n, off)
                sy, sz = ref.share_y(y, n, sel), ref.share_z(filt.state(), n, sel)
                assert sy <= 1.0 and sz <= 1.0, (name, rows, n, off, sy, sz)
                worst_y, worst_z, worst_d = max(worst_y, sy), max(worst_z, sz), max(worst_d, ref.share_beyond_rounding(y, n, sel))
        filt.close()
    print(f"\nsos {name}: worst share of the bound: rows {worst_y:.3f} (beyond the float32 rounding, of 16 e_ref + 2^-50 G: {worst_d:.3f}), "
          f"state {worst_z:.3f}")


@pytest.mark.parametrize("name", sr.SETS)
def test_any_split_of_a_stream_carries_the_state(sdr, gpu_ctx, refs, bufs, name):
    ref = refs[name]
    filt = sdr.RowSos(sr.S, ref.sos, ctx=gpu_ctx)
    worst = 0.0
    for n in (2 * sr.TILE + 3, 6149):
        for cuts in ((1,), (sr.TILE - 1,), (700, 700 + sr.TILE + 1)):
            filt.reset()
            edges = (0,) + cuts + (n,)
            y = np.concatenate([run(filt, bufs, ref.x[:, lo:hi], OFFSETS[i % 3]) for i, (lo, hi) in enumerate(zip(edges, edges[1:]))], axis=1)
            sy, sz = ref.share_y(y, n), ref.share_z(filt.state(), n)
            assert sy <= 1.0 and sz <= 1.0, (name, n, cuts, sy, sz)
            worst = max(worst, sy, sz)
    filt.close()
    print(f"\nsos {name}: worst share of the bound over the splits {worst:.3f}")


def test_in_place_meter_mode_and_state_round_trip(sdr, gpu_ctx, refs, bufs):
    ref = refs["ellip8"]
    xin, _ = bufs
    filt = sdr.RowSos(sr.S, ref.sos, ctx=gpu_ctx)
    for n in (513, 6149):
        x = ref.x[:, :n]
        filt.reset()
        y = run(filt, bufs, x, (1, 3))
        z = filt.state()
        # in place: the same bits, the guards between the rows untouched
        filt.reset()
        p, st = xin.place(x, 1, n + 5)
        filt.process_dev(p, st, p, st, n)
        got, rest = xin.fetch()
        assert np.array_equal(got.view(np.uint32), y.view(np.uint32)) and np.all(rest == sr.GUARD)
        assert np.array_equal(filt.state(), z)
        # no output: nothing moves but the state
        filt.reset()
        assert run(filt, bufs, x, (3, 0), y=False) is None
        assert np.array_equal(filt.state(), z)
        # the state set from the host is the state the next call starts from
        mid = n // 3
        zi = ref.zf(mid)
        filt.set_state(zi)
        assert np.array_equal(filt.state(), zi)
        tail = run(filt, bufs, x[:, mid:], (0, 0))
        bound = 2.0 ** -24 * np.abs(ref.y64[:, mid:n]) + ref.slack(n)[:, mid:]
        assert np.all(np.abs(tail.astype(np.float64) - ref.y64[:, mid:n]) <= bound)
        assert ref.share_z(filt.state(), n) <= 1.0
        # host rows
        filt.reset()
        assert np.array_equal(filt.run(x).view(np.uint32), y.view(np.uint32)) and np.array_equal(filt.state(), z)
    filt.close()


@pytest.mark.parametrize("n", (700, 6149))
def test_a_nan_takes_the_rest_of_its_row_and_no_other(sdr, gpu_ctx, refs, bufs, n):
    ref = refs["k_weighting"]
    filt = sdr.RowSos(sr.S, ref.sos, ctx=gpu_ctx)
    x = ref.x[:, :n].copy()
    clean = run(filt, bufs, x)
    zc = filt.state()
    x[1, 100] = np.nan
    filt.reset()
    y = run(filt, bufs, x)
    z = filt.state()
    for s in (0, 2):
        assert np.array_equal(y[s].view(np.uint32), clean[s].view(np.uint32)) and np.array_equal(z[s], zc[s])
    assert np.array_equal(y[1, :100].view(np.uint32), clean[1, :100].view(np.uint32))
    assert np.all(np.isnan(y[1, 100:])) and np.all(np.isnan(z[1]))
    filt.close()


def test_live_object_refuses_bad_calls(sdr, gpu_ctx):
    """SDR_EINVAL from the C side with a live object, before any launch: the state stays as it was"""
    lib = gpu_ctx.lib
    buf = sdr.DeviceBuffer(gpu_ctx, 1 << 16)
    filt = sdr.RowSos(3, sdr.design.k_weighting_sos(), ctx=gpu_ctx)
    try:
        h, p = filt._open(), buf.ptr
        z = np.arange(12, dtype=np.float64).reshape(3, 2, 2) + 0.5
        filt.set_state(z)
        q = p + 4 * 4096
        for args, word in (((None, 64, q, 64, 64), "x is NULL"), ((p, 64, q, 64, 0), "n="), ((p, 64, q, 64, -1), "n="), ((p, 2 ** 31, q, 2 ** 31, 2 ** 31), "n="),
                           ((p, 63, q, 64, 64), "x_stride"), ((p, 64, q, 63, 64), "y_stride"), ((p + 2, 64, q, 64, 64), "aligned"),
                           ((p, 64, q + 1, 64, 64), "aligned"), ((p, 64, p + 4 * 32, 64, 64), "overlap"), ((p, 64, p, 65, 64), "overlap")):
            assert lib.sdr_sos_process_dev(h, *args) == -1 and word in lib.sdr_last_error().decode(), (args, lib.sdr_last_error())
            with pytest.raises(ValueError):
                filt.process_dev(*args)
        host = np.zeros((3, 64), np.float32)
        assert lib.sdr_sos_run(h, None, host.ctypes.data, 64, 64) == -1 and lib.sdr_sos_run(h, host.ctypes.data, host.ctypes.data, 63, 64) == -1
        assert lib.sdr_sos_run(h, host.ctypes.data, None, 64, 0) == -1
        assert lib.sdr_sos_state(h, None) == -1 and lib.sdr_sos_set_state(h, None) == -1
        ms = (ctypes.c_float * 3)()
        assert lib.sdr_sos_stage_ms(h, ms) == -1 and "no timed call" in lib.sdr_last_error().decode()
        with pytest.raises(ValueError):
            filt.set_state(np.zeros((3, 2)))
        assert np.array_equal(filt.state(), z)
        filt.set_timing(True)
        filt.process_dev(p, 64, p, 64, 64)
        assert set(filt.stage_ms()) == {"reduce", "carry", "apply"}
    finally:
        filt.close()
        buf.free()
