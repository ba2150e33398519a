#!/usr/bin/env python3
"""Time the stereo blend / noise mute path with HIP events on the context stream, at the shapes
8 x 786 432 and 96 x 30 720 audio samples (streams x samples per block):

  audio         sdr_audio_out_dev: de-emphasis of L and R into f32 rows and int16 PCM (tools/audio_stage_time.py's call)
  audio_blend   sdr_audio_blend_dev: the same with a gain ramp per stream
  update        sdr_blend_update_dev on `streams` spectra of nfft / 2 + 1 bins
  rx / rx_blend a stereo receiver's block (u8 IQ on the device, 50 complex samples per audio sample)
                without and with blend

and, with --table, what a stereo receiver with blend measures for synth.fm_iq at input SNRs of
40, 30, 20, 10, 0 and -40 dB: the pilot ratio and the noise floor (10 log10 of mpx_quality's
noise_floor) of four blocks of 51 200 -- the figures a mute default would rest on.  One JSON line.

  python tools/blend_time.py [--reps 100] [--warmup 10] [--rx-reps 10] [--no-rx] [--table]
"""
import argparse
import json

import numpy as np

from _blocktime import copy_gbs, event_ms, rtsdr

SHAPES = ((8, 786_432), (96, 30_720))
TAU = 75e-6
NFFT = 1024


def stats(ms):
    us = np.asarray(ms) * 1e3
    return {"best_us": round(float(us.min()), 2), "median_us": round(float(np.median(us)), 2)}


def stage_times(ctx, S, n, reps, warmup):
    lib, h = ctx.lib, ctx.handle
    rng = np.random.default_rng(0)
    D = rtsdr.DeviceBuffer
    left = D.from_array(ctx, (0.3 * rng.standard_normal((S, n))).astype(np.float32))
    right = D.from_array(ctx, (0.3 * rng.standard_normal((S, n))).astype(np.float32))
    lo, ro, pcm = D(ctx, 4 * S * n), D(ctx, 4 * S * n), D(ctx, 4 * S * n)
    state = D.from_array(ctx, np.zeros((S, 2)))
    gains = D.from_array(ctx, np.tile(np.array([0.2, 0.7, 1.0, 0.9]), (S, 1)))
    b, den = rtsdr.design.deemphasis_coeffs(TAU, 48e3)
    bp = rtsdr._lib.f64p(np.ascontiguousarray(b))

    def plain():
        rtsdr._lib.check(lib.sdr_audio_out_dev(h, left.ptr, right.ptr, n, n, S, bp, float(den[1]), state.ptr, lo.ptr, ro.ptr,
                                               pcm.ptr, 2 * n), "sdr_audio_out_dev")

    def blended():
        rtsdr.audio_blend_dev(left.ptr, right.ptr, n, n, S, gains.ptr, b=b, a=den, state_ptr=state.ptr, left_out_ptr=lo.ptr,
                              right_out_ptr=ro.ptr, pcm_ptr=pcm.ptr, ctx=ctx)

    nb = NFFT // 2 + 1
    power = D.from_array(ctx, rng.uniform(0.5, 1.5, (S, nb)).astype(np.float32))
    ctl = rtsdr.BlendControl(S, ctx=ctx)
    t_plain, t_blend, t_upd = event_ms(ctx, [plain, blended, lambda: ctl.update_dev(power.ptr, nb, nb, 240e3)], reps, warmup)
    out = {"audio": stats(t_plain), "audio_blend": stats(t_blend), "update": stats(t_upd)}
    out["audio_blend_over_audio"] = round(out["audio_blend"]["median_us"] / out["audio"]["median_us"], 3)
    for buf in (left, right, lo, ro, pcm, state, gains, power):
        buf.free()
    ctl.close()
    return out


def rx_times(ctx, S, n, reps, warmup):
    B = 50 * n                                       # rf_decim 10 x audio_decim 5
    one = rtsdr.synth.fm_iq(min(B, 1_536_000), seed=3, dtype=np.uint8)
    iq = rtsdr.DeviceBuffer.from_array(ctx, np.tile(np.resize(one, 2 * B), (S, 1)))
    out = {}
    for name, kw in (("rx", {}), ("rx_blend", dict(blend=True, blend_nfft=NFFT))):
        rx = rtsdr.Receiver(S, B, stereo=True, iq_dtype=np.uint8, deemphasis=TAU, ctx=ctx, **kw)
        (ms,) = event_ms(ctx, [lambda: rx.process_dev(iq.ptr, B)], reps, warmup)
        out[name] = stats(ms)
        rx.close()
    out["rx_blend_over_rx"] = round(out["rx_blend"]["median_us"] / out["rx"]["median_us"], 4)
    iq.free()
    return out


def snr_table(ctx, blocks=4, B=51_200):
    snrs = (40.0, 30.0, 20.0, 10.0, 0.0, -40.0)
    iq = np.stack([rtsdr.synth.fm_iq(blocks * B, seed=70 + i, snr_db=s, dtype=np.uint8) for i, s in enumerate(snrs)])
    rx = rtsdr.Receiver(len(snrs), B, stereo=True, iq_dtype=np.uint8, deemphasis=TAU, blend=True, blend_nfft=NFFT, ctx=ctx)
    rows = [{"snr_db": s, "pilot_snr_db": [], "noise_floor_db": [], "stereo_gain": []} for s in snrs]
    for k in range(blocks):
        rx.process(np.ascontiguousarray(iq[:, 2 * k * B:2 * (k + 1) * B]), fetch=["left_de"])
        st = rx.blend_state()
        with np.errstate(divide="ignore"):
            nf = 10.0 * np.log10(st.noise_floor)
        for i, r in enumerate(rows):
            r["pilot_snr_db"].append(round(float(st.pilot_snr_db[i]), 2))
            r["noise_floor_db"].append(round(float(nf[i]), 2))
            r["stereo_gain"].append(round(float(st.stereo_gain[i]), 4))
    rx.close()
    return {"block_complex": B, "blocks": blocks, "nfft": NFFT, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rx-reps", type=int, default=10)
    ap.add_argument("--no-rx", action="store_true")
    ap.add_argument("--table", action="store_true")
    a = ap.parse_args()
    ctx = rtsdr.get_context()
    out = {"tau": TAU, "nfft": NFFT, "reps": a.reps, "warmup": a.warmup, "copy_gbs": round(copy_gbs(ctx), 1), "shapes": []}
    for S, n in SHAPES:
        row = {"streams": S, "n": n}
        row.update(stage_times(ctx, S, n, a.reps, a.warmup))
        if not a.no_rx:
            row.update(rx_times(ctx, S, n, a.rx_reps, 2))
        out["shapes"].append(row)
    if a.table:
        out["snr_table"] = snr_table(ctx)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
