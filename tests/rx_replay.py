"""A per-stage f64 replay of the block receiver (sdr_rx, csrc/rx.hip) for tests/test_rx_shapes.py.

For each output row the receiver materialises, the reference is the oracle's primitive of that
stage alone (oracle/fm_oracle.py: lfilter_fir, lfilter_decim, resample, fm_demod_arctan,
fm_pll_c) run on the rows the device produced as that stage's INPUT -- model/fmMonoBlock.py:86-170
and model/fmRDSblock.py:133-204 statement by statement, each statement fed the device's own
operands.  Every filter state, the demod phase and both PLL states are carried in f64 from block
to block and per stream; decimation restarts at each block, as lfilter(...)[::D] does in the
reference loops.  The PLLs therefore see inputs of identical signs on both sides and no sign-flip
window (tests/test_span.py) is needed: every sample of every block compares at the tight bounds.

The decimations and every tap array are arguments (the oracle's own block loops hard-code
10 / 5 / 151).  Fed the oracle's rows instead of a device's, the replay reproduces the oracle's
block loops (tests/test_rx_shapes.py::test_replay_reproduces_the_oracle_block_loops, on the CPU).
"""
import math

import numpy as np

RDS_UP, RDS_DOWN = 19, 80                            # model/fmRDSblock.py:184-199
PLL_INIT = (0.0, 0.0, 1.0, 0.0, 1.0, 0.0)            # model/fmMonoBlock.py:76, model/fmRDSblock.py:96
STEREO_PLL = dict(freq=19e3, Fs=240e3, ncoScale=2.0, phaseAdjust=0.0, normBandwidth=0.01)    # fmMonoBlock.py:119
RDS_PLL = dict(freq=114e3, Fs=240e3, ncoScale=0.5, phaseAdjust=math.pi / 3.3 - math.pi / 1.5,
               normBandwidth=0.001)                                                        # fmRDSblock.py:167
NCO_ROWS = ("nco", "nco_i", "nco_q")
STEREO_ROWS = ("bpf_recovery", "bpf_extraction", "nco", "stereo", "left", "right")
RDS_ROWS = ("extract", "pre_pll", "nco_i", "nco_q", "lpf_i", "lpf_q", "resample_i", "resample_q", "rrc_i", "rrc_q")


def lengths(B, rf_decim=10, audio_decim=5):
    """(M, A, R) of a block of B complex samples: demod, audio and RDS-rate samples per row"""
    M = -(-B // rf_decim)
    return M, -(-M // audio_decim), -(-(M * RDS_UP) // RDS_DOWN)


class _Stream:
    """one stream's carried states"""

    def __init__(self, taps):
        z = lambda name: np.zeros(len(taps[name]) - 1)   # noqa: E731
        self.zi = {"rf_i": z("rf"), "rf_q": z("rf"), "audio": z("audio")}
        for name in ("pilot", "stereo_bpf", "stereo_lpf"):
            if name in taps:
                self.zi[name] = z(name)
        if "rds_extract" in taps:
            self.zi.update(rds_extract=z("rds_extract"), rds_square=z("rds_square"),
                           lpf_i=z("rds_lpf"), lpf_q=z("rds_lpf"), anti_i=z("rds_anti"), anti_q=z("rds_anti"),
                           rrc_i=z("rds_rrc"), rrc_q=z("rds_rrc"))
        self.phase = 0.0
        self.pll = {"stereo": list(PLL_INIT), "rds": list(PLL_INIT)}


class Replay:
    """replay = Replay(oracle, S, taps, rf_decim, audio_decim); ref = replay.block(iq, rows) per block.

    taps: {"rf", "audio"[, "pilot", "stereo_bpf", "stereo_lpf"][, "rds_extract", "rds_square",
    "rds_lpf", "rds_anti", "rds_rrc"]} -> f64 tap arrays (the receiver's filter names); the stereo
    and the RDS chains are replayed when their taps are given.  pll_fn: oracle.fm_pll_c by default."""

    def __init__(self, oracle, nstreams, taps, rf_decim=10, audio_decim=5, pll_fn=None):
        self.o = oracle
        self.taps = {k: np.asarray(v, dtype=np.float64) for k, v in taps.items()}
        self.rf_decim, self.audio_decim = int(rf_decim), int(audio_decim)
        self.stereo = "pilot" in self.taps
        self.rds = "rds_extract" in self.taps
        self.pll_fn = pll_fn if pll_fn is not None else oracle.fm_pll_c
        self.streams = [_Stream(self.taps) for _ in range(int(nstreams))]

    @property
    def names(self):
        return ["demod", "audio"] + (list(STEREO_ROWS) if self.stereo else []) + (list(RDS_ROWS) if self.rds else [])

    def block(self, iq, rows):
        """One block.  iq: (S, 2 B) interleaved I, Q, already normalised ((u8 - 128) / 128 as
        model/fmRDSblock.py:59); rows: {name: (S, n)}, the rows each stage reads (a device's, or the
        oracle's).  Returns {name: [per stream f64 reference row]} for every name in self.names."""
        out = {name: [] for name in self.names}
        for s, st in enumerate(self.streams):
            row = lambda name: np.asarray(rows[name][s], dtype=np.float64)   # noqa: E731
            for name, ref in self._stream_block(st, np.asarray(iq[s], dtype=np.float64), row).items():
                out[name].append(ref)
        return out

    def state(self):
        """(demod phase [S], stereo PLL [S, 6], RDS PLL [S, 6]) after the last block: Receiver.state()'s shape"""
        return (np.array([st.phase for st in self.streams]),
                np.array([st.pll["stereo"] for st in self.streams], dtype=np.float64),
                np.array([st.pll["rds"] for st in self.streams], dtype=np.float64))

    def _stream_block(self, st, iq, row):
        o, t, zi = self.o, self.taps, st.zi
        r = {}
        # model/fmMonoBlock.py:86-98: RF FIR, [::rf_decim], arctan demod
        i_ds, zi["rf_i"] = o.lfilter_decim(t["rf"], iq[0::2], zi["rf_i"], self.rf_decim)
        q_ds, zi["rf_q"] = o.lfilter_decim(t["rf"], iq[1::2], zi["rf_q"], self.rf_decim)
        r["demod"], st.phase = o.fm_demod_arctan(i_ds, q_ds, st.phase)
        demod = row("demod")
        M = len(demod)
        # :101-105
        r["audio"], zi["audio"] = o.lfilter_decim(t["audio"], demod, zi["audio"], self.audio_decim)
        if self.stereo:
            # :117, :119, :151, :155-162, :166-170 (the intended combiner)
            r["bpf_recovery"], zi["pilot"] = o.lfilter_fir(t["pilot"], demod, zi["pilot"])
            r["bpf_extraction"], zi["stereo_bpf"] = o.lfilter_fir(t["stereo_bpf"], demod, zi["stereo_bpf"])
            r["nco"], _, st.pll["stereo"] = self._pll(row("bpf_recovery"), st.pll["stereo"], STEREO_PLL)
            mixed = np.multiply(row("nco")[0:M], row("bpf_extraction")) * 2
            r["stereo"], zi["stereo_lpf"] = o.lfilter_decim(t["stereo_lpf"], mixed, zi["stereo_lpf"], self.audio_decim)
            r["left"] = (row("audio") + row("stereo")) / 2
            r["right"] = (row("audio") - row("stereo")) / 2
        if self.rds:
            # model/fmRDSblock.py:156, :161-164, :167, :173-182, :184-199, :202-204
            r["extract"], zi["rds_extract"] = o.lfilter_fir(t["rds_extract"], demod, zi["rds_extract"])
            ext = row("extract")
            r["pre_pll"], zi["rds_square"] = o.lfilter_fir(t["rds_square"], np.square(ext), zi["rds_square"])
            r["nco_i"], r["nco_q"], st.pll["rds"] = self._pll(row("pre_pll"), st.pll["rds"], RDS_PLL)
            for c in ("i", "q"):
                mixed = np.multiply(ext, row("nco_" + c)[0:M]) * 2
                r["lpf_" + c], zi["lpf_" + c] = o.lfilter_fir(t["rds_lpf"], mixed, zi["lpf_" + c])
                r["resample_" + c], zi["anti_" + c] = o.resample(r["lpf_" + c], t["rds_anti"], zi["anti_" + c],
                                                                RDS_UP, RDS_DOWN)
                r["rrc_" + c], zi["rrc_" + c] = o.lfilter_fir(t["rds_rrc"], row("resample_" + c), zi["rrc_" + c])
        return r

    def _pll(self, x, state, cfg):
        return self.pll_fn(x, cfg["freq"], cfg["Fs"], list(state), cfg["ncoScale"], cfg["phaseAdjust"],
                           cfg["normBandwidth"])
