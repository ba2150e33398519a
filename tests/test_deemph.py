"""FM de-emphasis and the device-side audio output stage (csrc/audio.hip): the first-order IIR
section sdr_iir1 / sdr_iir1_dev (a parallel scan), sdr_audio_out_dev (filter + interleaved int16
PCM) and the receiver's tail stage (sdr_rx_set_deemph, sdr_rx_pcm).

The reference has no de-emphasis; parity is against scipy.signal.lfilter in f64 on the same f32
samples.  Bound (G = (|b0| + |b1|) / (1 - |a1|) * max|x|, the section's largest output):
    |y - y_ref| <= 2^-24 |y_ref| + 1e-12 G          one f32 rounding + the f64 allowance
    |zf - zf_ref| <= 1e-12 G
f32 accumulation cannot meet it; a scan that loses a wave or tile carry misses it by orders of
magnitude on the slow pole (p^64 = 0.97 there, 2e-8 at 75 us).
"""
import ctypes

import numpy as np
import pytest
from scipy import signal

TILE = 2048          # samples per workgroup (csrc/sdr_launch.h SDR_IIR_TILE)
SLOW = (np.array([2.5e-4, 2.5e-4]), -0.9995)
ALT = (np.array([0.5, -0.3]), 0.9)


def coeff_sets(sdr):
    out = {}
    for name, tau in (("75us", 75e-6), ("50us", 50e-6)):
        b, a = sdr.design.deemphasis_coeffs(tau, 48e3)
        out[name] = (b, float(a[1]))
    out["slow"] = SLOW
    out["alternating"] = ALT
    return out


def gain(b, a1, x):
    x = np.asarray(x, dtype=np.float64)
    return (abs(b[0]) + abs(b[1])) / (1.0 - abs(a1)) * float(np.max(np.abs(x[np.isfinite(x)])))


def ref_iir(b, a1, x32, zi=0.0):
    y, zf = signal.lfilter(b, [1.0, a1], np.asarray(x32, dtype=np.float32).astype(np.float64), zi=[zi])
    return y, float(zf[0])


def check_rows(y, y_ref, G, what=""):
    y = np.asarray(y, dtype=np.float64)
    err = np.abs(y - y_ref)
    lim = 2.0 ** -24 * np.abs(y_ref) + 1e-12 * G
    worst = int(np.argmax(err - lim))
    print(f"{what}: max |err| {err.max():.3e} (G {G:.3e}); tightest at {worst}: err {err[worst]:.3e}, bound {lim[worst]:.3e}")
    assert np.all(err <= lim), what


def pcm_rule(x):
    """The stage's PCM rule on f32 samples: v = x * 16384.0f; NaN -> 0; saturate; else truncate."""
    x = np.asarray(x, dtype=np.float32)
    v = x * np.float32(16384.0)
    nan = np.isnan(v)
    v = np.where(nan, np.float32(0), v)
    out = np.where(v >= 32767, 32767, np.where(v <= -32768, -32768, np.trunc(np.clip(v, -40000, 40000))))
    return np.where(nan, 0, out).astype(np.int16)


def interleave(left, right):
    out = np.empty(left.shape[:-1] + (2 * left.shape[-1],), dtype=np.int16)
    out[..., 0::2] = pcm_rule(left)
    out[..., 1::2] = pcm_rule(right)
    return out


# ---- CPU: the design ---------------------------------------------------------------
@pytest.mark.parametrize("tau", [50e-6, 75e-6])
def test_deemphasis_coeffs_match_bilinear(sdr, tau):
    fs = 48e3
    b, a = sdr.design.deemphasis_coeffs(tau, fs)
    wca = 2.0 * fs * np.tan(1.0 / (2.0 * fs * tau))
    rb, ra = signal.bilinear([wca], [1.0, wca], fs)
    assert b.shape == (2,) and a.shape == (2,) and a[0] == 1.0
    assert np.max(np.abs(b - rb)) <= 1e-15 and np.max(np.abs(a - ra)) <= 1e-15
    assert abs(b.sum() / a.sum() - 1.0) <= 1e-15                      # DC gain 1
    w = 2.0 * np.pi * (1.0 / (2.0 * np.pi * tau)) / fs                  # the corner, rad / sample
    h = (b[0] + b[1] * np.exp(-1j * w)) / (1.0 + a[1] * np.exp(-1j * w))
    assert abs(abs(h) - 1.0 / np.sqrt(2.0)) <= 1e-12


def test_deemphasis_defaults(sdr):
    b, a = sdr.design.deemphasis_coeffs()
    b2, a2 = sdr.design.deemphasis_coeffs(75e-6, 48e3)
    assert np.array_equal(b, b2) and np.array_equal(a, a2)
    with pytest.raises(ValueError):
        sdr.design.deemphasis_coeffs(0.0, 48e3)


def test_iir1_argument_errors_before_any_device_work(sdr):
    with pytest.raises(NotImplementedError):
        sdr.iir1([1.0, 0.5, 0.25], [1.0, 0.5], np.ones(4))            # second order
    with pytest.raises(NotImplementedError):
        sdr.iir1([1.0], [1.0, 0.5], np.ones(4, dtype=complex))
    with pytest.raises(ValueError):
        sdr.iir1([1.0, 0.0], [1.0, 0.5], np.ones(4), zi=np.zeros(2))  # zi shape
    with pytest.raises(NotImplementedError):
        sdr.lfilter([1.0, 0.0], [1.0, 0.5], np.ones(4))               # lfilter stays FIR-only


def test_receiver_names_cover_the_new_rows(sdr):
    from importlib import import_module
    _lib = import_module("real-time-software-defined-radio_amd._lib")
    assert _lib.RX_OUTPUTS[-3:] == ("audio_de", "left_de", "right_de")
    assert _lib.RX_OUTPUTS.index("rrc_q") == 17                       # the earlier rows keep their numbers


# ---- GPU: sdr_iir1 ------------------------------------------------------------------
LENGTHS = (1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 100_003)


@pytest.fixture(scope="module")
def noise():
    rng = np.random.default_rng(2024)
    return rng.standard_normal(100_003).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["75us", "50us", "slow", "alternating"])
def test_iir1_matches_scipy(sdr, gpu_ctx, noise, name):
    b, a1 = coeff_sets(sdr)[name]
    for n in LENGTHS:
        x = noise[:n]
        G = gain(b, a1, x)
        for zi in (None, 0.37 * G):
            y_ref, zf_ref = ref_iir(b, a1, x, 0.0 if zi is None else zi)
            if zi is None:
                y = sdr.iir1(b, [1.0, a1], x)
            else:
                y, zf = sdr.iir1(b, [1.0, a1], x, zi=[zi])
                assert zf.shape == (1,) and abs(zf[0] - zf_ref) <= 1e-12 * G, (name, n)
            assert y.dtype == np.float64 and y.shape == (n,)
            check_rows(y, y_ref, G, f"{name} n={n} zi={zi}")


@pytest.mark.gpu
def test_iir1_long_row(sdr, gpu_ctx):
    """More than 512 tiles: the carry launch's lanes chain more tiles than they hold in registers."""
    b, a1 = SLOW
    n = 520 * TILE + 5
    x = np.random.default_rng(7).standard_normal(n).astype(np.float32)
    G = gain(b, a1, x)
    y_ref, zf_ref = ref_iir(b, a1, x, 0.1 * G)
    y, zf = sdr.iir1(b, [1.0, a1], x, zi=[0.1 * G])
    check_rows(y, y_ref, G, "long row")
    assert abs(zf[0] - zf_ref) <= 1e-12 * G


def run_iir1_dev(sdr, ctx, x, stride, b, a1, zi, alias):
    """sdr_iir1_dev on the rows of x (S, n) laid out `stride` floats apart; returns (y (S, n), zf,
    the padding floats after each output row)."""
    S, n = x.shape
    D = sdr.DeviceBuffer
    host = np.full((S, stride), np.float32(7.0))
    host[:, :n] = x
    dx = D.from_array(ctx, host)
    dy = D.from_array(ctx, np.full((S, stride), np.float32(-3.0)))
    dzi = D.from_array(ctx, np.asarray(zi, dtype=np.float64))
    dzf = dzi if alias else D.from_array(ctx, np.zeros(S))
    bb = np.ascontiguousarray(b, dtype=np.float64)
    rc = ctx.lib.sdr_iir1_dev(ctx.handle, dx.ptr, n, stride, S, bb.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                              float(a1), dzi.ptr, dzf.ptr, dy.ptr, stride)
    from importlib import import_module
    import_module("real-time-software-defined-radio_amd._lib").check(rc, "sdr_iir1_dev")
    y = dy.download(S * stride).reshape(S, stride)
    zf = dzf.download(S, dtype=np.float64)
    for buf in {dx, dy, dzi, dzf}:
        buf.free()
    return y[:, :n], zf, y[:, n:]


@pytest.mark.gpu
@pytest.mark.parametrize("n,stride,alias", [(5000, 5003, True), (2 * TILE + 52, 2 * TILE + 56, False), (100, 128, True)])
def test_iir1_dev_streams_strides_and_states(sdr, gpu_ctx, noise, n, stride, alias):
    """3 streams, stride > n (16-B aligned rows and not), distinct non-zero zi, zf aliasing zi or
    not; the floats between the rows are not written."""
    b, a1 = SLOW
    x = np.stack([noise[k * 7001:k * 7001 + n] for k in range(3)])
    G = gain(b, a1, x)
    zi = np.array([0.25, -0.5, 0.125]) * G
    y, zf, pad = run_iir1_dev(sdr, gpu_ctx, x, stride, b, a1, zi, alias)
    assert np.all(pad == np.float32(-3.0))
    for s in range(3):
        y_ref, zf_ref = ref_iir(b, a1, x[s], zi[s])
        check_rows(y[s], y_ref, G, f"stream {s}")
        assert abs(zf[s] - zf_ref) <= 1e-12 * G


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["slow", "75us"])
def test_iir1_chained_blocks_equal_one_pass(sdr, gpu_ctx, noise, name):
    b, a1 = coeff_sets(sdr)[name]
    lens = [1, 7, 1024, 3071, 5]
    x = noise[:sum(lens)]
    G = gain(b, a1, x)
    y_ref, zf_ref = ref_iir(b, a1, x)
    z, out, pos = np.zeros(1), [], 0
    for m in lens:
        y, z = sdr.iir1(b, [1.0, a1], x[pos:pos + m], zi=z)
        out.append(y)
        pos += m
    check_rows(np.concatenate(out), y_ref, G, f"{name} chained")
    assert abs(z[0] - zf_ref) <= 1e-12 * G


@pytest.mark.gpu
@pytest.mark.parametrize("n,k", [(5000, 3000), (100, 37), (TILE + 10, TILE - 1)])
def test_iir1_nan_poisons_only_the_rest_of_its_stream(sdr, gpu_ctx, noise, n, k):
    b, a1 = SLOW
    x = np.stack([noise[s * 6000:s * 6000 + n] for s in range(3)]).copy()
    G = gain(b, a1, x)
    x[1, k] = np.nan
    y, zf, _ = run_iir1_dev(sdr, gpu_ctx, x, n + 4, b, a1, np.zeros(3), False)
    y_ref1, _ = ref_iir(b, a1, x[1])
    assert np.all(np.isnan(y_ref1[k:])) and np.all(np.isfinite(y_ref1[:k]))     # scipy's behaviour
    assert np.all(np.isnan(y[1, k:])) and np.isnan(zf[1])
    if k:
        check_rows(y[1, :k], y_ref1[:k], G, "before the NaN")
    for s in (0, 2):
        y_ref, zf_ref = ref_iir(b, a1, x[s])
        check_rows(y[s], y_ref, G, f"stream {s}")
        assert abs(zf[s] - zf_ref) <= 1e-12 * G


# ---- GPU: sdr_audio_out_dev -----------------------------------------------------------
def audio_rows(noise, n):
    """(2, n) left and right rows in (-1, 1) with runs of +-2.0 (saturation) in both streams and
    a NaN late in stream 1's right row."""
    L = np.stack([0.3 * noise[s * 4000:s * 4000 + n] for s in range(2)]).astype(np.float32)
    R = np.stack([0.3 * noise[50_000 + s * 4000:50_000 + s * 4000 + n] for s in range(2)]).astype(np.float32)
    L[0, 100:400] = 2.0
    R[0, 700:1000] = -2.0
    L[1, 1200:1500] = -2.0
    R[1, n - 20] = np.nan
    return L, R


@pytest.mark.gpu
@pytest.mark.parametrize("tau", [75e-6, 50e-6])
def test_audio_out_rows_pcm_and_state(sdr, gpu_ctx, noise, tau):
    n = TILE + 452
    L, R = audio_rows(noise, n)
    b, a = sdr.design.deemphasis_coeffs(tau, 48e3)
    st = np.zeros((2, 2))
    o = sdr.audio_out(L, R, b=b, a=a, state=st)
    assert o["pcm"].dtype == np.int16 and o["pcm"].shape == (2, 2 * n)
    assert np.array_equal(o["pcm"], interleave(o["left"], o["right"]))          # bit for bit
    assert o["pcm"].max() == 32767 and o["pcm"].min() == -32768                 # the runs saturate
    assert np.all(o["pcm"][1, 1::2][n - 20:] == 0) and np.all(np.isnan(o["right"][1, n - 20:]))
    for s in range(2):
        for ch, x in enumerate((L, R)):
            y_ref, zf_ref = ref_iir(b, a[1], x[s])
            ok = np.isfinite(y_ref)
            G = gain(b, a[1], x[s])
            check_rows(o["left" if ch == 0 else "right"][s][ok], y_ref[ok], G, f"stream {s} ch {ch}")
            assert (np.isnan(zf_ref) and np.isnan(st[s, ch])) or abs(st[s, ch] - zf_ref) <= 1e-12 * G
    # the PCM alone, from the same start state, is the same PCM
    o2 = sdr.audio_out(L, R, b=b, a=a, state=np.zeros((2, 2)), rows=False)
    assert set(o2) == {"pcm"} and np.array_equal(o2["pcm"], o["pcm"])


@pytest.mark.gpu
def test_audio_out_mono_on_both_channels(sdr, gpu_ctx, noise):
    n = 3000
    L, _ = audio_rows(noise, n)
    b, a = sdr.design.deemphasis_coeffs(75e-6, 48e3)
    o = sdr.audio_out(L, None, b=b, a=a)
    assert set(o) == {"left", "pcm"}
    assert np.array_equal(o["pcm"], interleave(o["left"], o["left"]))
    y_ref, _ = ref_iir(b, a[1], L[1])
    check_rows(o["left"][1], y_ref, gain(b, a[1], L[1]), "mono stream 1")


@pytest.mark.gpu
def test_audio_out_without_filter_is_the_host_writer(sdr, gpu_ctx, noise):
    """b = NULL: the PCM of in-range data equals tests/test_live.py's to_pcm (the reference's int16
    writer); out-of-range and NaN samples follow the stage's rule."""
    from test_live import to_pcm
    n = TILE + 77
    L = np.stack([0.2 * noise[:n], 0.15 * noise[n:2 * n]]).astype(np.float32)
    R = np.stack([0.2 * noise[3 * n:4 * n], 0.15 * noise[4 * n:5 * n]]).astype(np.float32)
    assert np.max(np.abs(L)) * 16384 < 32767 and np.max(np.abs(R)) * 16384 < 32767
    o = sdr.audio_out(L, R, rows=False)
    for s in range(2):
        assert np.array_equal(o["pcm"][s], to_pcm(L[s], R[s]))
    L2, R2 = audio_rows(noise, n)
    o = sdr.audio_out(L2, R2)
    assert np.array_equal(o["pcm"], interleave(L2, R2))
    assert np.array_equal(o["left"], L2) and np.array_equal(o["right"], R2, equal_nan=True)
    o = sdr.audio_out(L2, None, rows=False)
    assert np.array_equal(o["pcm"], interleave(L2, L2))


@pytest.mark.gpu
def test_argument_errors_raise_value_error(sdr, gpu_ctx):
    from importlib import import_module
    check = import_module("real-time-software-defined-radio_amd._lib").check
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    buf = sdr.DeviceBuffer(gpu_ctx, 4096)
    p = buf.ptr
    dp = ctypes.POINTER(ctypes.c_double)
    good = np.array([0.1, 0.1])

    def iir(n=16, xs=16, S=2, b=good, a1=-0.8, ys=16):
        bb = None if b is None else np.ascontiguousarray(b, dtype=np.float64).ctypes.data_as(dp)
        check(lib.sdr_iir1_dev(h, p, n, xs, S, bb, a1, None, None, p + 2048, ys))

    def audio(n=16, stride=16, S=2, b=good, a1=-0.8, state=p + 3072, lo=p + 1024, pcm=p + 2048, ps=32, right=p + 512,
              ro=None):
        bb = None if b is None else np.ascontiguousarray(b, dtype=np.float64).ctypes.data_as(dp)
        check(lib.sdr_audio_out_dev(h, p, right, n, stride, S, bb, a1, state, lo, ro, pcm, ps))

    iir()
    audio()
    gpu_ctx.synchronize()
    bad = [dict(n=0), dict(S=0), dict(xs=15), dict(ys=15), dict(b=[np.nan, 0.1]), dict(b=[0.1, np.inf]),
           dict(a1=np.nan), dict(a1=1.0000001), dict(a1=-1.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            iir(**kw)
    bad = [dict(n=0), dict(S=0), dict(stride=15), dict(ps=31), dict(b=[np.nan, 0.1]), dict(a1=np.inf), dict(a1=-1.01),
           dict(state=None), dict(lo=None, pcm=None), dict(right=None, ro=p + 1536)]
    for kw in bad:
        with pytest.raises(ValueError):
            audio(**kw)
    audio(b=None, state=None)                                        # no filter needs no state
    gpu_ctx.synchronize()
    buf.free()
    for a1 in (1.5, np.nan):
        with pytest.raises(ValueError):
            sdr.iir1([0.1, 0.1], [1.0, a1], np.ones(8))


# ---- GPU: the receiver's tail stage ---------------------------------------------------
BLK = 51_200
TAU = 75e-6


@pytest.fixture(scope="module")
def iq_blocks(sdr):
    return np.stack([sdr.synth.fm_iq(3 * BLK, seed=40 + s, dtype=np.uint8) for s in range(2)])


class Follower:
    """scipy over the concatenation of the receiver's own rows, block by block (the state
    carried in f64 as lfilter's zf)."""

    def __init__(self, sdr, S, names, tau=TAU):
        self.b, a = sdr.design.deemphasis_coeffs(tau, 48e3)
        self.a1 = float(a[1])
        self.z = {n: np.zeros(S) for n in names}

    def check(self, outs, pcm=None, stereo=True):
        for name in self.z:
            x, y = outs[name], outs[name + "_de"]
            for s in range(x.shape[0]):
                y_ref, self.z[name][s] = ref_iir(self.b, self.a1, x[s], self.z[name][s])
                check_rows(y[s], y_ref, max(gain(self.b, self.a1, x[s]), 1e-30), f"{name}_de stream {s}")
        if pcm is not None:
            want = interleave(outs["left_de"], outs["right_de"]) if stereo else interleave(outs["audio_de"], outs["audio_de"])
            assert pcm.dtype == np.int16 and np.array_equal(pcm, want)


def blocks_of(iq, B, k):
    return np.ascontiguousarray(iq[:, 2 * k * B:2 * (k + 1) * B])


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", [False, True])
def test_receiver_deemphasis_rows_and_pcm(sdr, gpu_ctx, iq_blocks, pipeline):
    """u8, 2 streams, stereo, three blocks of 51 200: the _de rows against scipy over the
    receiver's own rows, pcm() bit for bit, every other output bit-identical to a receiver
    without the stage; then reset() repeats the first block."""
    kw = dict(stereo=True, iq_dtype=np.uint8, pipeline=pipeline)
    rx = sdr.Receiver(2, BLK, deemphasis=TAU, **kw)
    plain = sdr.Receiver(2, BLK, **kw)
    assert [n for n in rx.outputs if n not in plain.outputs] == ["audio_de", "left_de", "right_de"]
    fol = Follower(sdr, 2, ("audio", "left", "right"))
    first = None
    for k in range(3):
        iq = blocks_of(iq_blocks, BLK, k)
        o = rx.process(iq, fetch=rx.outputs)
        p = plain.process(iq, fetch=plain.outputs)
        for name in plain.outputs:
            assert np.array_equal(o[name], p[name]), name
        pcm = rx.pcm()
        assert pcm.shape == (2, 2 * rx.A)
        fol.check(o, pcm)
        for name in ("audio_de", "left_de", "right_de"):
            assert np.array_equal(rx.output(name), o[name])            # sdr_rx_fetch of the same rows
        if k == 0:
            first = ({n: v.copy() for n, v in o.items()}, pcm.copy())
    rx.reset()
    o = rx.process(blocks_of(iq_blocks, BLK, 0), fetch=rx.outputs)
    for name in ("audio_de", "left_de", "right_de", "left"):
        assert np.array_equal(o[name], first[0][name]), name
    assert np.array_equal(rx.pcm(), first[1])
    # the default outputs gain the de-emphasised rows; without the stage they are unchanged
    assert list(rx.process(blocks_of(iq_blocks, BLK, 1))) == ["audio", "left", "right", "audio_de", "left_de", "right_de"]
    assert list(plain.process(blocks_of(iq_blocks, BLK, 1))) == ["audio", "left", "right"]


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", [False, True])
def test_receiver_deemphasis_through_submit(sdr, gpu_ctx, iq_blocks, pipeline):
    kw = dict(stereo=True, iq_dtype=np.uint8, pipeline=pipeline, depth=2)
    rx = sdr.Receiver(2, BLK, deemphasis=TAU, **kw)
    plain = sdr.Receiver(2, BLK, **kw)
    got, ref = [], []
    for k in range(3):
        iq = blocks_of(iq_blocks, BLK, k)
        got.append(rx.submit(iq, fetch=rx.outputs))
        ref.append(plain.submit(iq, fetch=plain.outputs))
    got = [o for o in got if o is not None] + rx.flush()
    ref = [o for o in ref if o is not None] + plain.flush()
    assert len(got) == 3 and len(ref) == 3
    fol = Follower(sdr, 2, ("audio", "left", "right"))
    for k, (o, p) in enumerate(zip(got, ref)):
        for name in plain.outputs:
            assert np.array_equal(o[name], p[name]), name
        fol.check(o, rx.pcm() if k == 2 else None)                   # pcm(): the latest block's


@pytest.mark.gpu
def test_receiver_deemphasis_mono_only(sdr, gpu_ctx, iq_blocks):
    rx = sdr.Receiver(2, BLK, iq_dtype=np.uint8, deemphasis=50e-6)
    assert "audio_de" in rx.outputs and "left_de" not in rx.outputs
    fol = Follower(sdr, 2, ("audio",), tau=50e-6)
    for k in range(2):
        o = rx.process(blocks_of(iq_blocks, BLK, k), fetch=["audio", "audio_de"])
        fol.check(o, rx.pcm(), stereo=False)
    with pytest.raises(ValueError):
        rx.output("left_de")
    proc = sdr.MonoBlockProcessor(BLK, iq_dtype=np.uint8, deemphasis=50e-6)
    a = proc.process(iq_blocks[0, :2 * BLK])
    assert np.array_equal(a.astype(np.float32), rx_first_block(sdr, iq_blocks))
    assert np.array_equal(proc.pcm(), interleave(a.astype(np.float32), a.astype(np.float32)))


def rx_first_block(sdr, iq_blocks):
    rx = sdr.Receiver(1, BLK, iq_dtype=np.uint8, deemphasis=50e-6)
    return rx.process(iq_blocks[:1, :2 * BLK], fetch=["audio_de"])["audio_de"][0]


@pytest.mark.gpu
def test_receiver_fetching_only_the_de_rows(sdr, gpu_ctx, iq_blocks):
    """A call that asks for the de-emphasised L / R alone gets the rows of a call that asks for
    everything (the stage's inputs are written whatever is kept); the stereo receiver's mono row
    is filtered only when it is asked for."""
    kw = dict(stereo=True, iq_dtype=np.uint8, deemphasis=TAU)
    rx, full = sdr.Receiver(2, BLK, **kw), sdr.Receiver(2, BLK, **kw)
    for k in range(2):
        iq = blocks_of(iq_blocks, BLK, k)
        o = rx.process(iq, fetch=["left_de", "right_de"])
        f = full.process(iq, fetch=full.outputs)
        assert np.array_equal(o["left_de"], f["left_de"]) and np.array_equal(o["right_de"], f["right_de"])
        assert np.array_equal(rx.pcm(), full.pcm())
        with pytest.raises(ValueError):
            rx.output("audio_de")                                      # not materialised by this block
        assert np.array_equal(full.output("audio_de"), f["audio_de"])


@pytest.mark.gpu
def test_receiver_deemphasis_on_spans(sdr, gpu_ctx):
    """The smallest span (327 680 complex -> 32 768 demod samples, A = 6 554: four tiles per row),
    two spans in a row: the state carries across spans."""
    B = 327_680
    iq = np.stack([sdr.synth.fm_iq(2 * B, seed=60 + s, dtype=np.uint8) for s in range(2)])
    kw = dict(stereo=True, iq_dtype=np.uint8)
    rx = sdr.Receiver(2, B, deemphasis=TAU, **kw)
    plain = sdr.Receiver(2, B, **kw)
    assert rx.A == 6554
    fol = Follower(sdr, 2, ("audio", "left", "right"))
    names = ["audio", "left", "right", "stereo", "audio_de", "left_de", "right_de"]
    for k in range(2):
        o = rx.process(blocks_of(iq, B, k), fetch=names)
        p = plain.process(blocks_of(iq, B, k), fetch=names[:4])
        for name in names[:4]:
            assert np.array_equal(o[name], p[name]), name
        fol.check(o, rx.pcm())


@pytest.mark.gpu
def test_stage_off_has_no_rows(sdr, gpu_ctx, iq_blocks):
    rx = sdr.Receiver(2, BLK, stereo=True, iq_dtype=np.uint8)
    assert "left_de" not in rx.outputs
    rx.process(blocks_of(iq_blocks, BLK, 0))
    for name in ("audio_de", "left_de", "right_de"):
        with pytest.raises(ValueError):
            rx.output(name)
        with pytest.raises(ValueError):
            rx.process(blocks_of(iq_blocks, BLK, 1), fetch=[name])
    with pytest.raises(ValueError):
        rx.pcm()
    with pytest.raises(ValueError):
        sdr.Receiver(1, BLK, mono=False, rds=True, deemphasis=TAU)
    proc = sdr.StereoBlockProcessor(BLK, iq_dtype=np.uint8)
    assert list(proc.process(iq_blocks[0, :2 * BLK])) == ["audio", "stereo", "left", "right"]
    proc = sdr.StereoBlockProcessor(BLK, iq_dtype=np.uint8, deemphasis=TAU)
    assert list(proc.process(iq_blocks[0, :2 * BLK])) == ["audio", "stereo", "left", "right", "audio_de", "left_de",
                                                         "right_de"]
