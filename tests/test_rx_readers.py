"""The stages that read a receiver's rows in place, behind every kind of receiver.

Every stage (RdsLinkBank / RdsSyncBank, RdsClockBank, RdsCarrierBank, RowSpectrum, RowMeter, RowSos,
LoudnessMeter) is pinned against its numpy specification in its own module, behind an un-pipelined
receiver with a host wait after each block.  Here the same stages run behind a pipelined receiver
(two and three row sets, the tiled and the generic front end, per-block and span lengths) with NO host
wait between the blocks, and everything they leave is compared bit for bit with the un-pipelined
twin: each kernel is deterministic and reads identical bytes.

The rule under test (include/sdr.h, sdr_rx_set_pipeline): work enqueued on the context stream between
process_dev(k) and process_dev(k+1) sees block k's rows, however far the host runs ahead.

  test_every_reader_in_every_mode        the mode matrix
  test_the_twin_equals_the_models        the twin's stages against the numpy models (existing bounds)
  test_a_reader_held_back_sees_its_block the ordering, with the context stream held back
  test_pipelined_spans                   row sets at span length (sign codes, long-call records)
"""
import functools
import time
import types

import numpy as np
import pytest
from scipy import signal

import rmeter_rows as rr
import sos_rows
from adverse_input import CASES, adverse_iq
from conftest import long_blocks

pytestmark = pytest.mark.gpu

S = 3
MODES = {"plain": dict(), "two_sets": dict(pipeline=True), "three_sets": dict(pipeline=True, depth=2),
         "two_sets_generic_fe": dict(pipeline=True)}
# rows the front half (FE, stages A and B), the PLLs and the NCO launch write
FRONT_ROWS = ("demod", "bpf_recovery", "pre_pll", "nco")


def _nq(mode_kw):
    return (3 if mode_kw.get("depth", 1) >= 2 else 2) if mode_kw.get("pipeline") else 1


def _taps(sdr, mode):
    """{} or the 51-tap RF filter of the generic front end (it runs on the context stream)"""
    if not mode.endswith("generic_fe"):
        return {}
    rf_b, au_b = sdr.design.mono_coeffs(51, 151)
    return dict(rf_coeff=rf_b, audio_coeff=au_b)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _differences(got, want):
    """the keys of two digests ({key: array or plain Python value}) whose values are not the same bits"""
    assert sorted(got) == sorted(want), (sorted(set(got) ^ set(want)))
    bad = []
    for key in got:
        g, w = got[key], want[key]
        ok = _same(g, w) if isinstance(w, np.ndarray) or isinstance(g, np.ndarray) else g == w
        if not ok:
            bad.append(key)
    return bad


def _meter_digest(d, key, meter):
    rec = meter.records()
    for f in rec._fields:
        d[f"{key}.{f}"] = getattr(rec, f)
    d[f"{key}.hist()"], d[f"{key}.windows()"] = meter.hist(), meter.windows()


def _d2d(ctx, dst, src, nbytes):
    """async on the context stream"""
    rc = ctx.lib.sdr_memcpy_d2d(ctx.handle, dst, src, int(nbytes))
    assert rc == 0, rc


def _phase(sdr, rx):
    """the carried demodulator phase per stream (a mono receiver has no PLL states to read)"""
    ph = np.empty(rx.S)
    sdr._lib.check(rx.lib.sdr_rx_state(rx.handle, sdr._lib.f64p(ph), None, None), "sdr_rx_state")
    return ph


def _rows_at(sdr, ctx, ptr, stride, n, nrows=S):
    """(nrows, n) float32 at a device pointer, rows stride floats apart (waits for the context stream)"""
    buf = np.empty(nrows * stride, dtype=np.float32)
    sdr._lib.check(ctx.lib.sdr_memcpy_d2h(ctx.handle, buf.ctypes.data, ptr, 4 * ((nrows - 1) * stride + n)), "d2h")
    return np.ascontiguousarray(buf.reshape(nrows, stride)[:, :n])


class _Copies:
    """Rows of the twin, uploaded: each output at its own pointer, the receiver's stride apart and at the
    receiver's alignment within 256 bytes"""

    def __init__(self, sdr, ctx, rx, rows):
        self.bufs, self.at = [], {}
        for name, x in rows.items():
            ptr, stride, n = rx.output_ptr(name)
            assert x.shape == (rx.S, n)
            off = ptr % 256
            host = np.zeros(rx.S * stride, dtype=np.float32)
            host.reshape(rx.S, stride)[:, :n] = x
            buf = sdr.DeviceBuffer(ctx, host.nbytes + 256)
            assert buf.ptr % 256 == 0
            buf.upload(host, offset=off)
            self.bufs.append(buf)
            self.at[name] = (buf.ptr + off, stride, n)

    def free(self):
        for b in self.bufs:
            b.free()


# ---- A. the mode matrix ------------------------------------------------------------------------------

B_A = 66_560                   # M 6 656, A 1 332, R 1 581 >= RdsLinkBank.MIN_N; 7 blocks hold a 100 ms loudness segment
NB_A = 7                       # 2 nq + 1 with three row sets


@functools.lru_cache(maxsize=None)
def _blocks_a(dt):
    import rtsdr as sdr
    iq = np.stack([sdr.synth.fm_iq(NB_A * B_A, seed=300 + s, dtype=dt, rds_groups=True) for s in range(S)])
    blocks = np.ascontiguousarray(np.stack([iq[:, 2 * k * B_A:2 * (k + 1) * B_A] for k in range(NB_A)]))
    assert all(not np.array_equal(blocks[k], blocks[k + 1]) for k in range(NB_A - 1))
    blocks.setflags(write=False)
    return blocks


class _Readers:
    """Every reader of a stereo + RDS receiver with de-emphasis (rx) and of a mono receiver without
    (mono), and the device buffers their rows go to"""

    def __init__(self, sdr, ctx, rx, mono, nb):
        self.sdr, self.ctx, self.rx, self.mono, self.nb = sdr, ctx, rx, mono, nb
        self.link = rx.rds_link()
        self.lsync = self.link.block_sync()
        self.clock = rx.rds_clock()
        self.csync = self.clock.block_sync()
        self.carrier = rx.rds_carrier()
        self.cclock = self.carrier.clock()
        self.ccsync = self.cclock.block_sync()
        self.spec = rx.mpx_spectrum(1024)
        self.mod = rx.modulation_meter()
        self.fast = rx.modulation_meter(window_s=0.002, nbins=64)      # 480 samples: windows complete
        self.aud = rx.audio_meter("left")
        self.maud = mono.audio_meter("audio")
        self.notch = rx.audio_filter(sdr.design.pilot_notch_sos())    # "left_de" into a buffer
        self.inplace = rx.audio_filter(sdr.design.pilot_notch_sos())  # "right_de" in place
        self.loud = rx.loudness_meter()
        self.mloud = mono.loudness_meter()
        assert rx.loudness_rows() == ("left_de", "right_de") and mono.loudness_rows() == ("audio",)
        _, self.mstride, self.M = rx.output_ptr("demod")
        _, self.astride, self.A = rx.output_ptr("left_de")
        self.srows = self.spec.rows(self.M)[1]
        self.spec_step = 4 * S * self.srows * self.spec.nbins
        self.audio_step = 4 * S * self.astride
        self.audio_used = 4 * ((S - 1) * self.astride + self.A)    # from the first row's start to the last row's end
        self.spec_out = sdr.DeviceBuffer(ctx, nb * self.spec_step)
        self.notch_out = sdr.DeviceBuffer(ctx, nb * self.audio_step)
        self.inplace_out = sdr.DeviceBuffer(ctx, nb * self.audio_step)
        for b in (self.spec_out, self.notch_out, self.inplace_out):
            b.zero()

    def _chain(self):
        self.lsync.process_links(self.link)
        self.clock.feed(self.csync)
        self.carrier.feed(self.cclock)
        self.cclock.feed(self.ccsync)

    def feed_rx(self, k):
        """block k's readers by process_rx: the rows are looked up at every call"""
        rx, mono = self.rx, self.mono
        self.link.process_rx(rx)
        self.clock.process_rx(rx)
        self.carrier.process_rx(rx)
        self._chain()
        assert self.spec.process_rx(rx, self.spec_out.ptr + k * self.spec_step) == self.srows
        self.mod.process_rx(rx)
        self.fast.process_rx(rx)
        self.aud.process_rx(rx, "left")
        self.maud.process_rx(mono, "audio")
        self.notch.process_rx(rx, "left_de", out_ptr=self.notch_out.ptr + k * self.audio_step)
        self.loud.process_rx(rx)
        self.mloud.process_rx(mono)
        self.inplace.process_rx(rx, "right_de")                   # after the loudness meter has read the row
        _d2d(self.ctx, self.inplace_out.ptr + k * self.audio_step, rx.output_ptr("right_de")[0], self.audio_used)

    def feed_copies(self, k, at, mono_at):
        """the same calls by process_dev, on uploaded copies ({name: (pointer, stride, n)})"""
        (pi, rs, R), (pq, _, _) = at["rrc_i"], at["rrc_q"]
        self.link.process_dev(pi, R, rs)
        self.clock.process_dev(pi, R, rs)
        self.carrier.process_dev(pi, pq, R, rs)
        self._chain()
        pd, ds, M = at["demod"]
        self.spec.process_dev(pd, M, ds, self.spec_out.ptr + k * self.spec_step)
        self.mod.process_dev(pd, ds, M)
        self.fast.process_dev(pd, ds, M)
        self.aud.process_dev(*at["left"])
        self.maud.process_dev(*mono_at["audio"])
        (pl, st, A), (pr, _, _) = at["left_de"], at["right_de"]
        self.notch.process_dev(pl, st, self.notch_out.ptr + k * self.audio_step, st, A)
        self.loud.process_dev(pl, pr, st, A)
        pm, ms, Am = mono_at["audio"]
        self.mloud.process_dev(pm, None, ms, Am)
        self.inplace.process_dev(pr, st, pr, st, A)
        _d2d(self.ctx, self.inplace_out.ptr + k * self.audio_step, pr, self.audio_used)

    def digest(self):
        """Everything the readers hold, after waiting for them: the last call's events, bits, records and
        rows, every carried state, every block's spectrum and filtered rows"""
        d = {}
        ev, status = self.link.events()
        d["link.events"], d["link.status"], d["link.counts"] = ev, status, self.link.counts
        for s in range(S):
            d[f"link.bits[{s}]"], d[f"link.diff[{s}]"] = self.link.bits(s)
        for key, bank in (("clock", self.clock), ("carrier.clock", self.cclock)):
            for s, b in enumerate(bank.bits()):
                d[f"{key}.bits[{s}]"] = b
            d[f"{key}.state"] = bank.state()
        for key, sync in (("link.sync", self.lsync), ("clock.sync", self.csync), ("carrier.sync", self.ccsync)):
            d[f"{key}.blocks"], d[f"{key}.state"] = sync.blocks(), sync.state()
        d["carrier.rows"], d["carrier.state"], d["carrier.moments"] = self.carrier.rows(), self.carrier.state(), self.carrier.moments()
        d["spectrum"] = self.spec_out.download(self.nb * self.spec_step // 4).reshape(self.nb, S, self.srows, self.spec.nbins)
        for key, m in (("modulation", self.mod), ("modulation.fast", self.fast), ("audio.left", self.aud), ("audio.mono", self.maud)):
            _meter_digest(d, key, m)
        for key, buf in (("notch.left_de", self.notch_out), ("notch.right_de", self.inplace_out)):
            d[key] = np.ascontiguousarray(buf.download(self.nb * self.audio_step // 4).reshape(self.nb, S, self.astride)[:, :, :self.A])
        d["notch.left_de.state"], d["notch.right_de.state"] = self.notch.state(), self.inplace.state()
        for key, m in (("loudness", self.loud), ("loudness.mono", self.mloud)):
            first, e = m.segments()
            d[f"{key}.first"], d[f"{key}.energies"] = first, e
        return d

    def close(self):
        for o in (self.lsync, self.csync, self.ccsync, self.cclock, self.link, self.clock, self.carrier, self.spec, self.mod, self.fast,
                  self.aud, self.maud, self.notch, self.inplace, self.loud, self.mloud):
            o.close()
        for b in (self.spec_out, self.notch_out, self.inplace_out):
            b.free()


def _receivers_a(sdr, ctx, dt, mode, **kw):
    kw = dict(MODES[mode], **_taps(sdr, mode), iq_dtype=dt, ctx=ctx, **kw)
    return sdr.Receiver(S, B_A, stereo=True, rds=True, deemphasis=75e-6, **kw), sdr.Receiver(S, B_A, **kw)


@functools.lru_cache(maxsize=None)
def _twin_a(dt, generic):
    """The un-pipelined twin: the blocks through process(), identical stage objects fed by process_dev from
    uploaded copies of the rows it returned.  Returns (the readers' digest, per block {name: rows} of the
    stereo receiver and of the mono one, the two receivers' state())."""
    import rtsdr as sdr
    ctx = sdr.get_context()
    mode = "two_sets_generic_fe" if generic else "plain"
    kw = dict(_taps(sdr, mode), iq_dtype=dt, ctx=ctx)
    rx, mono = sdr.Receiver(S, B_A, stereo=True, rds=True, deemphasis=75e-6, **kw), sdr.Receiver(S, B_A, **kw)
    readers = _Readers(sdr, ctx, rx, mono, NB_A)
    blocks = _blocks_a(dt)
    rows, mrows = [], []
    for k in range(NB_A):
        rows.append(rx.process(blocks[k], fetch=rx.outputs))
        mrows.append(mono.process(blocks[k], fetch=mono.outputs))
        up, mup = _Copies(sdr, ctx, rx, rows[k]), _Copies(sdr, ctx, mono, mrows[k])
        readers.feed_copies(k, up.at, mup.at)
        ctx.synchronize()
        up.free()
        mup.free()
    out = readers.digest(), rows, mrows, rx.state(), _phase(sdr, mono)
    readers.close()
    rx.close()
    mono.close()
    return out


@pytest.mark.parametrize("dt", (np.uint8, np.float32), ids=("u8", "f32"))
@pytest.mark.parametrize("mode", list(MODES))
def test_every_reader_in_every_mode(sdr, gpu_ctx, mode, dt):
    """Seven consecutive blocks of three stations through process_dev, every reader's process_rx after each,
    no host wait before the end: every record, event list, bit row, histogram, state vector, float row and
    spectrum equals the un-pipelined twin's bit for bit, and so do the receiver's own rows of the last nq
    blocks (through pointers held from output_ptr) and its state()."""
    blocks = _blocks_a(dt)
    want, rows, mrows, state, mstate = _twin_a(dt, mode.endswith("generic_fe"))
    nq = _nq(MODES[mode])
    assert NB_A == 2 * 3 + 1 >= 2 * nq + 1
    rx, mono = _receivers_a(sdr, gpu_ctx, dt, mode)
    readers = _Readers(sdr, gpu_ctx, rx, mono, NB_A)
    d = sdr.DeviceBuffer.from_array(gpu_ctx, blocks)
    gpu_ctx.synchronize()
    step = blocks[0].nbytes
    held = []
    try:
        for k in range(NB_A):
            rx.process_dev(d.ptr + k * step, B_A)
            mono.process_dev(d.ptr + k * step, B_A)
            readers.feed_rx(k)
            held.append(({n: rx.output_ptr(n) for n in rx.outputs}, {n: mono.output_ptr(n) for n in mono.outputs}))
        gpu_ctx.synchronize()
        got = readers.digest()
        assert len({held[k][0]["demod"][0] for k in range(NB_A)}) == nq      # the row sets did alternate
        bad = _differences(got, want)
        assert not bad, (mode, "the readers differ from the twin's in", bad)
        # the receiver's own outputs: unchanged by the readers, but for the row filtered in place
        for k in range(NB_A - nq, NB_A):
            for ptrs, ref in ((held[k][0], rows[k]), (held[k][1], mrows[k])):
                for name, (ptr, stride, n) in ptrs.items():
                    expect = want["notch.right_de"][k] if name == "right_de" and ref is rows[k] else ref[name]
                    assert _same(_rows_at(sdr, gpu_ctx, ptr, stride, n), expect), (mode, name, k)
        for name in rx.outputs:
            if name != "right_de":
                assert _same(rx.output(name), rows[-1][name]), (mode, name)
        for a, b in zip(rx.state() + (_phase(sdr, mono),), state + (mstate,)):
            assert _same(a, b), mode
    finally:
        readers.close()
        d.free()
        rx.close()
        mono.close()


@pytest.mark.parametrize("dt", (np.uint8, np.float32), ids=("u8", "f32"))
def test_the_twin_equals_the_models(sdr, gpu_ctx, dt):
    """What the mode matrix compares with is itself the specification's: the twin's rows through the numpy
    models (RowMeterModel, sos_model, LoudnessModel, RdsSymbolClock, RdsCarrierPhase, RdsBlockSync), checked
    with the stages' own helpers and bounds (tests/rmeter_rows.py, tests/sos_rows.py, tests/test_loudness.py;
    the RDS stages with equality)."""
    from test_loudness import check as loudness_check
    want, rows, mrows, _, _ = _twin_a(dt, False)
    cat = lambda rr_, name: np.concatenate([r[name] for r in rr_], axis=1)   # noqa: E731
    # RDS: carrier -> clock -> sync, clock -> sync; the link bank's sync on the link bank's own scanned bits
    for s in range(S):
        carrier, cclock, ccsync = sdr.RdsCarrierPhase(), sdr.RdsSymbolClock(), sdr.RdsBlockSync()
        clock, csync = sdr.RdsSymbolClock(), sdr.RdsBlockSync()
        for k in range(NB_A):
            y = carrier.process(rows[k]["rrc_i"][s], rows[k]["rrc_q"][s])
            cbits = cclock.process(y)
            crec = ccsync.process(cbits)
            bits = clock.process(rows[k]["rrc_i"][s])
            rec = csync.process(bits)
        eq = np.array_equal
        assert eq(want["carrier.rows"][s], y) and want["carrier.state"][s] == carrier.state(), s
        assert want["carrier.moments"][s] == carrier.moments(), s
        assert eq(want[f"carrier.clock.bits[{s}]"], cbits) and want["carrier.clock.state"][s] == cclock.state(), s
        assert want["carrier.sync.blocks"][s] == crec and want["carrier.sync.state"][s] == ccsync.state(), s
        assert eq(want[f"clock.bits[{s}]"], bits) and want["clock.state"][s] == clock.state(), s
        assert want["clock.sync.blocks"][s] == rec and want["clock.sync.state"][s] == csync.state(), s
        links, lsync = sdr.RdsLinkLayer(), sdr.RdsBlockSync()
        for k in range(NB_A):
            diff = links.process(rows[k]["rrc_i"][s])["diff"]
            lrec = lsync.process(diff if k == 0 else diff[27:])
        assert eq(want[f"link.diff[{s}]"], diff), s
        assert want["link.sync.blocks"][s] == lrec and want["link.sync.state"][s] == lsync.state(), s
    # the meters
    rx, mono = _receivers_a(sdr, gpu_ctx, dt, "plain")
    for key, meter, rr_, name in (("modulation", rx.modulation_meter(), rows, "demod"),
                                  ("modulation.fast", rx.modulation_meter(window_s=0.002, nbins=64), rows, "demod"),
                                  ("audio.left", rx.audio_meter("left"), rows, "left"), ("audio.mono", mono.audio_meter("audio"), mrows, "audio")):
        model, bound = sdr.RowMeterModel(S, meter.window, meter.nbins, meter.scale, meter.limit), rr.SumBound(S)
        for k in range(NB_A):
            model.process(rr_[k][name])
            bound.take(rr_[k][name])
        rec = sdr.RowMeterRecord(*(want[f"{key}.{f}"] for f in sdr.RowMeterRecord._fields))
        rr.check((rec, want[f"{key}.hist()"], want[f"{key}.windows()"]), (model.records(), model.hist(), model.windows()), bound, key)
    assert want["modulation.fast.total_windows"].tolist() == [NB_A * rx.M // 480] * S
    rx.close()
    mono.close()
    # the notch: tests/sos_rows.py's bound, its noise term from a long-double loop over these rows
    sos = sdr.design.pilot_notch_sos()
    for key, name in (("notch.left_de", "left_de"), ("notch.right_de", "right_de")):
        x = cat(rows, name)
        y_ld, _ = sos_rows.longdouble_loop([sos], x, ())
        ref = signal.sosfilt(sos, x.astype(np.float64), axis=-1)
        _, zf = sdr.sos_model(sos, x)
        noise = np.maximum.accumulate(np.abs(ref.astype(np.longdouble) - y_ld[0]).astype(np.float64), axis=1)
        slack = 16.0 * noise + 2.0 ** -50 * sos_rows.gain_bound(sos, x)
        got = np.concatenate(list(want[key]), axis=1).astype(np.float64)
        assert got.shape == ref.shape and np.all(np.abs(got - ref) <= 2.0 ** -24 * np.abs(ref) + slack), key
        assert np.all(np.abs(want[key + ".state"] - zf) <= slack[:, -1][:, None, None]), key
    # loudness: the stereo meter read right_de before the in-place notch
    for key, channels, rr_ in (("loudness", ("left_de", "right_de"), rows), ("loudness.mono", ("audio",), mrows)):
        model = sdr.LoudnessModel(S, len(channels))
        for k in range(NB_A):
            model.process([rr_[k][c] for c in channels])
        assert model.energies().shape[2] == NB_A * 1332 // 4800 == 1

        kept = types.SimpleNamespace(nstreams=S, channels=len(channels), segment=4800, cap=4096,     # what the check reads of a meter
                                     segments=lambda key=key: (want[f"{key}.first"], want[f"{key}.energies"]))
        loudness_check(kept, model, key)


# ---- B. the ordering -----------------------------------------------------------------------------------

B_B = 15_360
GIB = 1 << 30
HOLD_MAX_COPIES = 64            # 64 GiB of copy traffic


@pytest.fixture(scope="module")
def hold_buffers(sdr, gpu_ctx):
    a, b = sdr.DeviceBuffer(gpu_ctx, GIB), sdr.DeviceBuffer(gpu_ctx, GIB)
    a.zero()
    _d2d(gpu_ctx, b.ptr, a.ptr, GIB)
    gpu_ctx.synchronize()
    yield a, b
    a.free()
    b.free()


def _hold(ctx, bufs, copies):
    """the hold: a chain of 1 GiB device-to-device copies on the context stream, to and fro"""
    a, b = bufs
    for i in range(copies):
        src, dst = (a, b) if i % 2 == 0 else (b, a)
        _d2d(ctx, dst.ptr, src.ptr, GIB)


def _hold_ms(sdr, ctx, bufs, copies):
    t = sdr._lib.Timer(ctx)
    e0, e1 = t.event(), t.event()
    t.record(e0)
    _hold(ctx, bufs, copies)
    t.record(e1)
    ctx.synchronize()
    ms = t.elapsed_ms(e0, e1)
    t.close()
    return ms


class _FrontReaders:
    """The readers of the rows a front half, the PLLs and the NCO launch overwrite: of a stereo + RDS receiver
    a meter on each of FRONT_ROWS and the multiplex spectrum, of a mono receiver a meter and a notch in place
    on "audio" (the filtered rows copied out at once: the row set turns)"""

    def __init__(self, sdr, ctx, rx, mono):
        self.ctx, self.mono = ctx, mono
        if mono:
            self.meters = {"audio": rx.audio_meter("audio", window_s=0.002)}
            self.sos = rx.audio_filter(sdr.design.pilot_notch_sos())
            _, stride, self.n = rx.output_ptr("audio")
        else:
            self.meters = {name: rx.modulation_meter(window_s=0.002, nbins=64) for name in FRONT_ROWS}
            self.spec = rx.mpx_spectrum(1024)
            _, stride, self.n = rx.output_ptr("demod")
            self.srows = self.spec.rows(self.n)[1]
        self.shape = (S, stride) if mono else (S, self.srows, self.spec.nbins)
        self.used = 4 * ((S - 1) * stride + self.n)               # from the first row's start to the last row's end
        self.out = sdr.DeviceBuffer(ctx, 4 * int(np.prod(self.shape)))
        self.out.zero()

    def feed_rx(self, rx):
        for name, m in self.meters.items():
            m.process_rx(rx, name)
        if self.mono:
            self.sos.process_rx(rx, "audio")
            _d2d(self.ctx, self.out.ptr, rx.output_ptr("audio")[0], self.used)
        else:
            self.spec.process_rx(rx, self.out.ptr)

    def feed_copies(self, at):
        for name, m in self.meters.items():
            m.process_dev(*at[name])
        if self.mono:
            pa, st, A = at["audio"]
            self.sos.process_dev(pa, st, pa, st, A)
            _d2d(self.ctx, self.out.ptr, pa, self.used)
        else:
            pd, ds, M = at["demod"]
            self.spec.process_dev(pd, M, ds, self.out.ptr)

    def digest(self):
        d = {}
        for name, m in self.meters.items():
            _meter_digest(d, f"RowMeter({name})", m)
        out = self.out.download(int(np.prod(self.shape))).reshape(self.shape)
        if self.mono:
            d["RowSos(audio) rows"], d["RowSos(audio) state"] = np.ascontiguousarray(out[:, :self.n]), self.sos.state()
        else:
            d["RowSpectrum(demod)"] = out
        return d

    def close(self):
        for o in (*self.meters.values(), self.sos if self.mono else self.spec):
            o.close()
        self.out.free()


@pytest.mark.parametrize("dt", (np.float32, np.uint8), ids=("f32", "u8"))
@pytest.mark.parametrize("depth", (1, 2), ids=("two_sets", "three_sets"))
@pytest.mark.parametrize("mono", (False, True), ids=("stereo_rds", "mono"))
def test_a_reader_held_back_sees_its_block(sdr, gpu_ctx, hold_buffers, mono, depth, dt):
    """process_dev(k); a hold on the context stream; the readers of block k's front-half rows; process_dev
    (k+1 .. k+nq); one wait.  The hold outlasts, ten times over, the host's nq calls plus the GPU's nq front
    halves and PLLs, so a front half of block k+nq that is not ordered after the readers overwrites their
    rows while the context stream is still held; the readers must equal the same readers on the twin's block k,
    bit for bit.  The hold's length is a precondition (asserted and printed), not something the result waits on:
    a correctly ordered receiver passes with any hold.

    One receiver per case, so that as few streams as can be are alive: the runtime shares a few hardware
    queues among all streams, and a front stream that shares the context stream's queue is held with it.
    Before sdr_rx_process_dev recorded the readers' event (ev_read) the three-row-set cases failed on an
    MI355X -- first difference RowMeter(demod) (stereo + RDS) and RowMeter(audio) (mono), block 6: the readers
    had read block 9 -- and the two-row-set cases passed (profiles/rxreaders/test_rx_readers_parent.txt)."""
    nq = depth + 1
    warm = 2 * nq                     # nq untimed calls (the first allocates), then nq timed ones; waited for
    nb = warm + 1 + nq
    k = warm
    iq = np.stack([sdr.synth.fm_iq(nb * B_B, seed=340 + s, dtype=dt) for s in range(S)])
    blocks = np.ascontiguousarray(np.stack([iq[:, 2 * j * B_B:2 * (j + 1) * B_B] for j in range(nb)]))
    assert all(not np.array_equal(blocks[j], blocks[j + 1]) for j in range(nb - 1))
    kw = dict(iq_dtype=dt, ctx=gpu_ctx) if mono else dict(stereo=True, rds=True, iq_dtype=dt, ctx=gpu_ctx)
    names = ["audio"] if mono else list(FRONT_ROWS)
    # the twin, its stages timed: block k's rows, and what nq front halves and PLLs take on the GPU
    twin = sdr.Receiver(S, B_B, **kw)
    twin.set_timing(True)
    ref = _FrontReaders(sdr, gpu_ctx, twin, mono)
    for j in range(k + 1):                                        # the readers carry state: every block up to k
        up = _Copies(sdr, gpu_ctx, twin, twin.process(blocks[j], fetch=names))
        ref.feed_copies(up.at)
        gpu_ctx.synchronize()
        up.free()
    ms = twin.stage_ms()
    gpu_ms = nq * sum(ms[st] for st in ("fe", "filters_of_demod", "rds_square", "pll"))
    want = ref.digest()
    ref.close()
    twin.close()

    rx = sdr.Receiver(S, B_B, pipeline=True, depth=depth, **kw)
    readers = _FrontReaders(sdr, gpu_ctx, rx, mono)
    d = sdr.DeviceBuffer.from_array(gpu_ctx, blocks)
    gpu_ctx.synchronize()
    step = blocks[0].nbytes
    try:
        # the warm-up, readers attached (a reader's first call makes its device object, which waits for the
        # device: it must not be the call behind the hold)
        host_ms = 0.0
        for j in range(warm):
            t0 = time.perf_counter()
            rx.process_dev(d.ptr + j * step, B_B)
            host_ms += 1e3 * (time.perf_counter() - t0) if j >= nq else 0.0
            readers.feed_rx(rx)
            gpu_ctx.synchronize()
        need = 10.0 * (host_ms + gpu_ms)
        copies, hold_ms = 1, _hold_ms(sdr, gpu_ctx, hold_buffers, 1)
        while hold_ms <= need and copies < HOLD_MAX_COPIES:
            copies *= 2
            hold_ms = _hold_ms(sdr, gpu_ctx, hold_buffers, copies)
        print(f"\nhold: {copies} x 1 GiB = {hold_ms:.2f} ms; needed > 10 x (host {host_ms:.3f} ms + GPU {gpu_ms:.3f} ms) = {need:.2f} ms"
              f"  [{'mono' if mono else 'stereo + RDS'}, {nq} row sets, {np.dtype(dt).name}]")
        assert hold_ms > need, f"a hold of {copies} GiB of copies takes {hold_ms:.2f} ms, not more than {need:.2f} ms"
        rx.process_dev(d.ptr + k * step, B_B)
        first = rx.output_ptr(names[0])[0]
        _hold(gpu_ctx, hold_buffers, copies)
        readers.feed_rx(rx)
        for j in range(k + 1, k + 1 + nq):
            rx.process_dev(d.ptr + j * step, B_B)
        assert rx.output_ptr(names[0])[0] == first                # block k+nq took block k's row set
        gpu_ctx.synchronize()
        bad = _differences(readers.digest(), want)
        assert not bad, (f"block {k}'s readers, held back behind {nq} more blocks, differ from the twin's: first in", bad[0], "in all", bad)
    finally:
        readers.close()
        d.free()
        rx.close()


# ---- D. a pipelined receiver on spans -----------------------------------------------------------------

S_D, B_D = 2, 327_720              # M 32 772: a ragged span (tests/test_rx_shapes.py)
NB_D = 7


@functools.lru_cache(maxsize=None)
def _blocks_d(adverse):
    import rtsdr as sdr
    if adverse:                    # solves leave round 0 while two row sets' work records are live
        iq = np.stack([adverse_iq(NB_D * B_D, 5 + s, **CASES["S"]) for s in range(S_D)])
    else:
        iq = np.stack([sdr.synth.fm_iq(NB_D * B_D, seed=360 + s, dtype=np.uint8) for s in range(S_D)])
    blocks = np.ascontiguousarray(np.stack([iq[:, 2 * k * B_D:2 * (k + 1) * B_D] for k in range(NB_D)]))
    blocks.setflags(write=False)
    return blocks


def _keep(lean):
    from test_span import NAMES, NCO_NAMES
    return [nm for nm in NAMES if not lean or nm not in NCO_NAMES + ("lpf_i", "lpf_q", "bpf_recovery", "pre_pll")]


@functools.lru_cache(maxsize=None)
def _twin_d(adverse, lean):
    """the un-pipelined span receiver over the same blocks, per block: {name: rows}, state(), the solver counters so far"""
    import rtsdr as sdr
    ctx = sdr.get_context()
    names = _keep(lean)
    blocks = _blocks_d(adverse)
    rx = sdr.Receiver(S_D, B_D, stereo=True, rds=True, iq_dtype=np.uint8, keep=names, ctx=ctx)
    d = sdr.DeviceBuffer.from_array(ctx, blocks)
    ctx.pll_stats(reset=True)
    rows, states, stats = [], [], []
    for k in range(NB_D):
        rx.process_dev(d.ptr + k * blocks[0].nbytes, B_D)
        rows.append({n: rx.output(n) for n in names})
        states.append(rx.state())
        stats.append(rx.pll_stats())
    out = rows, states, stats
    d.free()
    rx.close()
    return out


@pytest.mark.parametrize("depth,lean,adverse", [(1, False, False), (1, True, False), (2, False, False), (2, True, False), (1, False, True),
                                                (2, True, True)])
def test_pipelined_spans(sdr, gpu_ctx, depth, lean, adverse):
    """2 nq + 1 (and up to seven) consecutive u8 blocks of M = 32 772 through a pipelined receiver's process_dev
    without host waits -- the row-set index also selects the PLLs' sign-code rows, the long calls' work
    records and the compact phase rows -- with every output kept and with the bench's lean keep set: one
    fetch mid-run, and after the last block the last nq blocks' row sets through pointers held from output_ptr;
    every materialised output and state() equal the un-pipelined receiver bit for bit, and every recurrence
    is accounted for.  On the adverse input (tests/adverse_input.py, S) solves leave round 0."""
    nq = depth + 1
    nb = 2 * nq + 1
    assert nb <= NB_D
    names = _keep(lean)
    blocks = _blocks_d(adverse)
    rows, states, stats = _twin_d(adverse, lean)
    rx = sdr.Receiver(S_D, B_D, stereo=True, rds=True, iq_dtype=np.uint8, pipeline=True, depth=depth, keep=names, ctx=gpu_ctx)
    d = sdr.DeviceBuffer.from_array(gpu_ctx, blocks)
    gpu_ctx.synchronize()
    gpu_ctx.pll_stats(reset=True)
    mid = nq                         # the first block that takes a row set a second time
    held = []
    try:
        for k in range(nb):
            rx.process_dev(d.ptr + k * blocks[0].nbytes, B_D)
            held.append({n: rx.output_ptr(n) for n in names})
            if k == mid:
                for n in names:
                    assert _same(rx.output(n), rows[k][n]), ("mid-run", n, k)
        gpu_ctx.synchronize()
        assert len({h["demod"][0] for h in held}) == nq
        for k in range(nb - nq, nb):
            for n, (ptr, stride, cnt) in held[k].items():
                assert _same(_rows_at(sdr, gpu_ctx, ptr, stride, cnt, S_D), rows[k][n]), (n, k)
        st = rx.pll_stats()
        print(f"\npipelined spans, {nq} row sets, lean={lean}, adverse={adverse}: solver counters {st}")
        M = -(-B_D // 10)
        assert st["recurrences"] == nb * S_D * 2 * long_blocks(M), st
        if adverse:
            assert sum(st[c] for c in ("spec_r1", "spec_r2", "long_stops", "long_tail", "sequential")) > 0, st
        else:
            assert st["long_guessed"] + st["long_chained"] == nb * S_D * 2 * long_blocks(M), st
        assert st == stats[nb - 1], (st, stats[nb - 1])            # the same solves as the twin's
        for a, b in zip(rx.state(), states[nb - 1]):
            assert _same(a, b)
    finally:
        d.free()
        rx.close()
