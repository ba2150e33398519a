"""Digest of the row blocks' outputs (GPU box), in the manner of tools/rx_digest.py: for a fixed
list of small Channelizer / FilterBank / RowResampler / Spectrum configurations -- aimed at what
the blocks share: the carried history, calls shorter than it, the seam between history and buffer,
the host-path staging -- one line per call with a SHA-256 (its first 16 hex digits) of the call's
whole output buffer, the unwritten floats between rows included, and the object's position.  Two
libraries compute the same thing when their outputs are identical line for line (SDR_LIB selects
the library; tools/build_dbg.sh builds another one).  Inputs are np.random.default_rng streams
with fixed seeds; nothing outside the repository is read.
usage: python tools/blocks_digest.py"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtsdr as sdr  # noqa: E402

CTX = sdr.get_context()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def capture(n, dt, seed):
    """n complex samples of interleaved IQ"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, 2 * n, dtype=np.uint8) if dt == np.uint8 else rng.standard_normal(2 * n, dtype=np.float32)


def decim_block(tag, obj, dt, calls, seed, shift=0):
    """a Channelizer / FilterBank through process_dev, the calls consecutive pieces of one
    capture that starts `shift` bytes into its device buffer; then one call through process"""
    iq = capture(sum(calls), dt, seed)
    es = 2 * iq.itemsize
    din = sdr.DeviceBuffer(CTX, iq.nbytes + shift + 16)
    din.upload(iq, shift)
    at = 0
    for k, n in enumerate(calls):
        stride = n // obj.decim + 3
        out = sdr.DeviceBuffer(CTX, obj.nch * stride * 8)
        out.zero()
        obj.process_dev(din.ptr + shift + at * es, n, out.ptr, stride)
        print(f"{tag} call {k} n={n} {sha(out.download(obj.nch * stride * 2))} pos={obj.position}")
        out.free()
        at += n
    n = calls[1]
    print(f"{tag} host n={n} {sha(obj.process(iq[:2 * n]))} pos={obj.position}")
    obj.close()
    din.free()


def ddc():
    for dt, name in ((np.float32, "f32"), (np.uint8, "u8")):
        for nch in (3, 9):                                  # one and two row tiles
            for shift in (0, 2) if dt == np.uint8 else (0,):    # u8: also 2 bytes off a 4-byte boundary
                ch = sdr.Channelizer(np.linspace(-0.4, 0.37, nch), 1.0, 4, taps=33, iq_dtype=dt, ctx=CTX)
                decim_block(f"ddc_{name}_nch{nch}_T33_D4_shift{shift}", ch, dt, [4, 28, 320, 4, 4096], 11 + nch, shift)
        ch = sdr.Channelizer([-0.3, 0.01, 0.25], 1.0, 64, taps=256, iq_dtype=dt, ctx=CTX)    # the one-column-block window
        decim_block(f"ddc_{name}_nch3_T256_D64", ch, dt, [64 * 16, 64 * 16], 17)


def pfb():
    for dt, name in ((np.float32, "f32"), (np.uint8, "u8")):
        for nbins, D, T, bins in ((12, 5, 36, [0, 5, 11, 5]), (96, 8, 768, None)):
            fb = sdr.FilterBank(nbins, 1.0, D, bins=bins, taps=T, iq_dtype=dt, ctx=CTX)
            decim_block(f"pfb_{name}_M{nbins}_D{D}_T{T}", fb, dt, [D, 7 * D, 64 * D, D, 640 * D], 23 + nbins)


def rsmp():
    rows = 3
    for cplx in (False, True):
        e = 2 if cplx else 1
        for U, D, T, calls in ((3, 4, 31, [4, 8, 4096]), (24, 25, 501, [25, 50, 2500]), (600, 599, 1201, [599, 1198])):
            tag = f"rsmp_{'complex' if cplx else 'real'}_{U}_{D}_T{T}"
            rs = sdr.RowResampler(rows, U, D, taps=T, complex=cplx, ctx=CTX)
            x = np.random.default_rng(31 + U).standard_normal((rows, e * sum(calls)), dtype=np.float32)
            at = 0
            for k, n in enumerate(calls):
                mo = rs.out_len(n)
                buf = np.full((rows, e * (n + 3)), np.nan, dtype=np.float32)      # in_stride = n + 3: the gaps are never read
                buf[:, :e * n] = x[:, e * at:e * (at + n)]
                din = sdr.DeviceBuffer.from_array(CTX, buf)
                out = sdr.DeviceBuffer(CTX, rows * (mo + 5) * 4 * e)
                out.zero()
                rs.process_dev(din.ptr, n, n + 3, out.ptr, mo + 5)
                print(f"{tag} call {k} n={n} {sha(out.download(rows * (mo + 5) * e))} pos={rs.position}")
                out.free()
                din.free()
                at += n
            n = calls[1]
            xin = x[:, :e * n].copy()
            y = rs.process(xin.view(np.complex64) if cplx else xin)
            print(f"{tag} host n={n} {sha(y)} pos={rs.position}")
            rs.close()


def spec():
    nfft, hop, navg = 256, 129, 3
    n = nfft + hop * 8
    for dt, name in ((np.float32, "f32"), (np.uint8, "u8")):
        iq = capture(n, dt, 41)
        sp = sdr.Spectrum(nfft, 1.0, hop=hop, navg=navg, iq_dtype=dt, ctx=CTX)
        print(f"spec_{name} run n={n} {sha(sp.run(iq))}")
        din = sdr.DeviceBuffer.from_array(CTX, iq)
        rows = sp.rows(n)[1]
        out = sdr.DeviceBuffer(CTX, rows * (nfft + 7) * 4)
        out.zero()
        sp.process_dev(din.ptr, n, out.ptr, nfft + 7)
        print(f"spec_{name} process_dev n={n} {sha(out.download(rows * (nfft + 7)))}")
        sp.close()
        out.free()
        din.free()


ddc()
pfb()
rsmp()
spec()
