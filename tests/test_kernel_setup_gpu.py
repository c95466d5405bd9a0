"""GPU: the set-up of the transcode kernels - what a wavefront does before its first real work: staging the frame, copying
the tables, requesting descriptors and rows.  The mantissa kernels issue those loads ahead of their first wait, a fixed number
per thread, each guarded by its index (decode_common.h stage_frame_fetch / stage_frame_store, the prologues of mant_kernel and
mantx_kernel; decode_wg_kernel stages through the same code); the parse kernel and the encoder's three keep their copy loops
(profiles/EXPERIMENTS.md) and are held to the same results.  The shapes here are the smallest at which such a prologue can go wrong: fewer streams than the eight XCD slots of the frame mapping and one more (1, 7, 9); frames of
128 bytes (most threads stage nothing), 1536 bytes (nw = the 384 threads of the mantissa kernels: a thread's second word is
padding only), 2560 bytes (two words a thread), 1670 bytes (44.1 kHz, not a multiple of 4: the masked tail word), and a batch
of 1536-byte frames in 2560-byte slots beside full ones (trim_staged_frame behind the staging stores).

Frames are the oracle encoder's on the harness's `music` content, so the decoder's bar is the one of
tests/test_full_size_gpu.py: one s16 step against the liba52 restatement with the reference's converter (one float32 ulp at
bias 384 is one step).  Everything else is exact: the engine's two paths byte for byte, the encoder against the oracle byte
for byte."""
import os

import numpy as np
import pytest

from tests import _decode_matrix as M
from tests import _harness as H
from tests import _mixed_sizes as X
from tests import _tools as T

pytestmark = pytest.mark.gpu

NS = (1, 7, 9)
SMAX = 9
# name -> (channels, bit rate, sample rate, frame bytes)
SIZES = {"128": (1, 32000, 48000, 128), "1536": (6, 384000, 48000, 1536), "2560": (6, 640000, 48000, 2560),
         "1670": (6, 384000, 44100, 1670)}
_BUILT = {}


def _restore(engine):
    engine.set_decode_mode(int(os.environ.get("AC3MI_DECODE_MODE", "0")))
    engine.set_encode_mode(0)
    engine.set_fixed_shape(1)


def _oracle_frames(name):
    """SMAX one-frame streams of the size: [SMAX][1][fb], each a fresh oracle encoder's first frame"""
    if ("frames", name) not in _BUILT:
        nch, rate, sr, fb = SIZES[name]
        out = np.zeros((SMAX, 1, fb), np.uint8)
        for s in range(SMAX):
            out[s] = H.orc_encode(H.gen_pcm(1, nch, seed=8100 + 17 * s + nch, kind="music"), nch, rate, sr, T.chmap_of(nch))
            assert X.own_size(out[s, 0]) == fb
        out.setflags(write=False)
        _BUILT["frames", name] = out
    return _BUILT["frames", name]


def _batch(name):
    """-> (frames [SMAX][1][slot], case): a size of SIZES, or "mixed": 1536-byte frames (streams 0, 2, ...) and 2560-byte ones
    in slots of 2560 bytes, 0xff behind the short ones (tests/_mixed_sizes.lay)"""
    if name != "mixed":
        nch = SIZES[name][0]
        return _oracle_frames(name), T.layout_of(nch) + (name,)
    if ("frames", name) not in _BUILT:
        short, full = _oracle_frames("1536"), _oracle_frames("2560")
        out = X.lay([[(full if s & 1 else short)[s, 0]] for s in range(SMAX)], 2560, 0xff)
        out.setflags(write=False)
        _BUILT["frames", name] = out
    return _BUILT["frames", name], (7, 1, name)


def _oracle_s16(name):
    """the restatement's s16 PCM of the batch, [SMAX][1][6][256][n_out], every frame read by its own size"""
    if ("s16", name) not in _BUILT:
        frames, case = _batch(name)
        L = H.orc()
        n_out = H.NFCHANS[case[0]] + case[1]
        want = np.zeros((SMAX, 1, 6, 256, n_out), np.int16)
        for s in range(SMAX):
            own = X.own_size(frames[s, 0])
            pcm, errs, oflags = H.orc_decode(np.ascontiguousarray(frames[s, :, :own]), case[0] | 16 * case[1], 1.0, 384.0)
            assert errs == 0
            for b in range(6):
                L.orc_convert_s16(H.P(np.ascontiguousarray(pcm[0, b]), H.fp), H.P(want[s, 0, b], H.i16p), oflags)
        want.setflags(write=False)
        _BUILT["s16", name] = want
    return _BUILT["s16", name]


# ---------------------------------------------------------------------------------------------------------------------
# staging

@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", list(SIZES) + ["mixed"])
def test_staging(engine, name, n):
    """ac3mi_decode_s16_batch of n one-frame streams under ac3mi_set_decode_mode 6 (mantx_kernel) and 4 (mant_kernel +
    the transform): PCM, overlap state, dither state and status byte for byte the same, with ac3mi_set_fixed_shape on and -
    for the 5.1 sizes, which are the ones it applies to - off; and within one s16 step of the restatement."""
    frames, case = _batch(name)
    frames, want = frames[:n], _oracle_s16(name)[:n]
    flags = case[0] | 16 * case[1]
    try:
        base = None
        for fixed in ((1, 0) if case[0] == 7 else (1,)):
            engine.set_fixed_shape(fixed)
            for mode in (6, 4):
                engine.set_decode_mode(mode)
                got = M.decode(engine, frames, case, flags, s16=True)
                what = "%s bytes, %d streams, mode %d, fixed shape %d" % (name, n, mode, fixed)
                assert not (got["status"] & 0x1ff).any(), (what, got["status"])
                step = int(np.abs(got["pcm"].astype(np.int32) - want).max())
                print("%s: largest difference from the restatement %d step(s)" % (what, step))
                assert step <= 1, what
                if base is None:
                    base = got
                    assert got["pcm"].any()
                M.same(got, base, what + " against mode 6 with the fixed shape")
    finally:
        _restore(engine)


# ---------------------------------------------------------------------------------------------------------------------
# stale LDS

def _lds_heavy(engine, frames):
    """two unrelated calls whose kernels fill their LDS with something else: the CRC sums of the frames, a loudness measurement"""
    import torch
    engine.crc_check_batch(torch.from_numpy(M.pad(frames)).cuda(), frames.shape[-1])
    pcm = torch.from_numpy(H.gen_pcm(SMAX, 6, seed=8300, kind="noise").reshape(SMAX, 1, 1536, 6)).cuda()
    engine.loudness_batch(48000, H.pkg().loudness_roles(7 | 16), pcm)
    engine.sync()


def test_nothing_is_read_before_it_is_written(engine):
    """the same decode and the same encode twice, LDS-heavy calls of other kernels between them: identical results.  A pad
    word or a table entry that a kernel read before its set-up had written it would hold what the call before left."""
    frames, case = _batch("mixed")
    pcm = H.gen_pcm(SMAX, 6, seed=8200, kind="bursts").reshape(SMAX, 1536, 6)
    try:
        for mode in (6, 4):
            engine.set_decode_mode(mode)
            first = M.decode(engine, frames, case, 7 | 16, s16=True)
            _lds_heavy(engine, frames)
            M.same(M.decode(engine, frames, case, 7 | 16, s16=True), first, "decode mode %d after other kernels" % mode)
        for pack in (1, 2):
            first = T.encode(engine, pcm, pack=pack)
            _lds_heavy(engine, frames)
            assert np.array_equal(T.encode(engine, pcm, pack=pack), first), "encode, packer %d, after other kernels" % pack
    finally:
        _restore(engine)


# ---------------------------------------------------------------------------------------------------------------------
# packer and search tables

ENC = {"5.1 384": (6, 384000), "2/0 192": (2, 192000), "1/0 64": (1, 64000)}
ENC_S = 65


def _enc_case(name, F):
    """-> (pcm [S][F*1536][nch], the oracle's frames [S][F][fb]): ENC_S one-frame streams, or three two-frame ones"""
    if ("enc", name, F) not in _BUILT:
        nch, rate = ENC[name]
        S = ENC_S if F == 1 else 3
        pcm = H.gen_pcm(S * F, nch, seed=8400 + nch + F, kind="bursts").reshape(S, F * 1536, nch)
        want = np.stack([H.orc_encode(pcm[s], nch, rate, 48000, T.chmap_of(nch)) for s in range(S)])
        want.setflags(write=False)
        _BUILT["enc", name, F] = (pcm, want)
    return _BUILT["enc", name, F]


@pytest.mark.parametrize("n", (1, ENC_S))
@pytest.mark.parametrize("name", list(ENC))
def test_packer_tables(engine, name, n):
    """ac3mi_encode_batch of n one-frame streams through the frame packer (ac3mi_set_encode_mode 1) and the block packer (2):
    every byte the oracle's - the quantiser and bit-count tables (packlut, bitlut), band_of_bin -, and both CRCs of every
    frame zero (crc_tab)."""
    import bench
    pcm, want = _enc_case(name, 1)
    try:
        for pack in (1, 2):
            got = T.encode(engine, pcm[:n], rate=ENC[name][1], pack=pack)
            differ = np.argwhere((got != want[:n]).any(axis=2))
            assert not len(differ), "%s, packer %d: frames %r differ from the oracle's" % (name, pack, differ[:8].tolist())
            assert bench.ac3_crc_ok(got.reshape(n, -1)) == 0, "%s, packer %d" % (name, pack)
    finally:
        _restore(engine)


@pytest.mark.parametrize("name", list(ENC))
def test_search_state_is_carried(engine, name):
    """three two-frame streams: the second frame's search starts from the first's offsets; bytes equal the oracle's"""
    pcm, want = _enc_case(name, 2)
    try:
        for pack in (1, 2):
            got = T.encode(engine, pcm, rate=ENC[name][1], pack=pack)
            assert np.array_equal(got, want), "%s, packer %d" % (name, pack)
    finally:
        _restore(engine)


# ---------------------------------------------------------------------------------------------------------------------
# transcode

@pytest.mark.parametrize("n", (1, 9))
def test_transcode(engine, n):
    """n one-frame 5.1 streams from fresh state: frames, status and the four state arrays are the same with
    ac3mi_set_fixed_shape on and off, and the frames are those of ac3mi_decode_s16_batch followed by ac3mi_encode_batch"""
    import torch
    pkg = H.pkg()
    frames = _oracle_frames("1536")[:n]
    dec = pkg.DecodeDesc(flags=7 | 16, level=1.0, bias=384.0, dynrng=1, acmod=7, lfeon=1, frame_bytes=1536)
    enc = pkg.EncodeDesc(48000, 384000, 6)
    src = torch.from_numpy(M.pad(frames)).cuda()

    def state():
        return (torch.zeros((n, 6, 128), dtype=torch.float32, device="cuda"), torch.ones((n,), dtype=torch.int16, device="cuda"),
                torch.zeros((n, 6, 256), dtype=torch.int16, device="cuda"), torch.full((n,), 40, dtype=torch.int32, device="cuda"))

    def host(*ts):
        return [np.ascontiguousarray(t.cpu().numpy()) for t in ts]

    names = "frames status delay lfsr last_samples csnroffst".split()
    try:
        res = []
        for fixed in (1, 0):
            engine.set_fixed_shape(fixed)
            st = state()
            out, status = engine.transcode_batch(dec, enc, src, st[0], st[1], H.CHMAP6, st[2], st[3])
            engine.sync()
            res.append(host(out, status, *st))
        for k, a, b in zip(names, *res):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), "%s: fixed shape on against off" % k
        assert not (res[0][1] & 0x1ff).any() and res[0][0].any()
        st = state()
        pcm, status = engine.decode_s16_batch(dec, src, st[0], st[1])
        out = engine.encode_batch(enc, pcm.view(n, 1, 1536, 6), H.CHMAP6, st[2], st[3])
        engine.sync()
        for k, a, b in zip(names, res[0], host(out, status, *st)):
            assert a.tobytes() == b.tobytes(), "%s: the transcode against decode-to-s16 followed by encode" % k
    finally:
        _restore(engine)
