"""fm_radio_gpu --deemph 50|75 --blend: the receiver's stereo blend in the live program (mode 0
stereo, sdr_rx_set_blend with its defaults and a 1 024-point spectrum).  The PCM is compared with
the Python receiver's with blend=True, block by block, by the acceptance of
tests/test_live_deemph.py (<= 1 LSB, < 1 % off)."""
import subprocess

import numpy as np
import pytest

from test_live import B, BIN
from test_live_deemph import accept


def test_blend_usage_errors():
    for args in (["--blend"], ["--blend", "--deemph", "75", "--mono"], ["--blend", "--deemph", "75", "--mode", "1"]):
        res = subprocess.run([BIN] + args, capture_output=True, text=True)
        assert res.returncode == 2 and "--blend" in res.stderr, args
    assert "[--deemph 50|75 [--blend]]" in subprocess.run([BIN, "--nonsense"], capture_output=True, text=True).stderr


def test_print_taps_is_unchanged_by_the_flag():
    plain = subprocess.run([BIN, "--print-taps"], capture_output=True, text=True, check=True).stdout
    res = subprocess.run([BIN, "--print-taps", "--deemph", "75", "--blend"], capture_output=True, text=True, check=True)
    assert res.stdout == plain


@pytest.mark.gpu
def test_live_blend_matches_the_python_receiver(sdr, gpu_ctx):
    nb = 3
    iq = sdr.synth.fm_iq(nb * B, seed=9, dtype=np.uint8)

    def run(*flags):
        res = subprocess.run([BIN, "--deemph", "75", *flags], input=iq.tobytes(), capture_output=True, check=True, timeout=120)
        return np.frombuffer(res.stdout, dtype=np.int16)

    pcm = run("--blend")
    assert pcm.shape == (nb * 2 * (B // 50),)
    rf, au = sdr.design.mono_coeffs(151, 151)
    rx = sdr.Receiver(1, B, stereo=True, iq_dtype=np.uint8, rf_coeff=rf, audio_coeff=au, deemphasis=75e-6, blend=True)
    ref, g = [], []
    for k in range(nb):
        rx.process(iq[None, 2 * k * B:2 * (k + 1) * B], fetch=["left_de"])
        ref.append(rx.pcm()[0])
        g.append(rx.blend_state().stereo_gain[0])
    accept(pcm, np.concatenate(ref).astype(np.int32))
    assert 0.0 < g[0] < g[1] < g[2] < 1.0                              # the ramp is in the compared blocks
    # without the flag the bytes are those of another run of the same program, and not the blended ones
    plain = run()
    assert np.array_equal(plain, run()) and plain.shape == pcm.shape and not np.array_equal(plain, pcm)
