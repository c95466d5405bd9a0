"""GPU parity of the packers' single-form quantiser (csrc/enc_mant.h: mant_quant_lut in contract, the exact quantisers
for blocks with a negative shift): both packers - one wavefront per frame (enc_packf_kernel) and one per audio block
(enc_packb_kernel) - against the oracle, byte for byte, on first-generation 5.1 content and on second-generation content
(decoded, then re-encoded), where reuse runs pull exponents below a block's shift and the out-of-contract path runs."""
import ctypes

import numpy as np
import pytest

from tests import _harness as H

pytestmark = pytest.mark.gpu


def _gpu_encode(engine, pcm_streams, mode):
    import torch
    pkg = H.pkg()
    desc = pkg.EncodeDesc(48000, 384000, 6)
    S, F = len(pcm_streams), pcm_streams[0].shape[0] // 1536
    pcm = torch.from_numpy(np.stack(pcm_streams).reshape(S, F, 1536, 6)).cuda()
    last = torch.zeros((S, 6, 256), dtype=torch.int16, device="cuda")
    csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
    engine.set_encode_mode(mode)
    try:
        out = engine.encode_batch(desc, pcm, H.CHMAP6, last, csnr)
        engine.sync()
    finally:
        engine.set_encode_mode(0)
    return out.cpu().numpy()[:, :, :desc.frame_bytes()]


def _second_generation(seeds, kind, frames):
    L = H.orc()
    out = []
    for seed in seeds:
        first = H.orc_encode(H.gen_pcm(frames, 6, seed=seed, kind=kind))
        dec, errs, oflags = H.orc_decode(first, 7 | 16 | 32, 1.0, 384.0)
        assert errs == 0
        s16 = np.zeros((frames * 6, 256, 6), np.int16)
        for f in range(frames):
            for b in range(6):
                L.orc_convert_s16(H.P(np.ascontiguousarray(dec[f, b]), H.fp), H.P(s16[f * 6 + b], H.i16p), oflags)
        out.append(s16.reshape(frames * 1536, 6))
    return out


def _negshift_count():
    L = H.orc()
    L.orc_ac3enc_debug_counts.argtypes = [ctypes.POINTER(ctypes.c_long)] * 2
    n = ctypes.c_long()
    L.orc_ac3enc_debug_counts(None, ctypes.byref(n))
    return n.value


@pytest.mark.parametrize("mode", [1, 2])
def test_first_generation_one_frame_streams(engine, mode):
    """The bench's shape: one-frame 5.1 / 48 kHz / 384 kbps streams of every content kind, every frame byte-exact."""
    kinds = ("tones", "noise", "quiet", "music", "bursts", "strobe")
    pcm = [H.gen_pcm(1, 6, seed=700 + s, kind=kinds[s % len(kinds)]) for s in range(48)]
    want = np.stack([H.orc_encode(p) for p in pcm])
    got = _gpu_encode(engine, pcm, mode)
    bad = [s for s in range(len(pcm)) if not np.array_equal(got[s], want[s])]
    assert not bad, "frames differ in streams %s" % bad


@pytest.mark.parametrize("mode", [1, 2])
def test_second_generation_takes_the_exact_path(engine, mode):
    negshift = 0
    for kind in ("bursts", "strobe", "music"):
        pcm = _second_generation(range(800, 806), kind, 3)
        n0 = _negshift_count()
        want = np.stack([H.orc_encode(p) for p in pcm])
        negshift += _negshift_count() - n0
        got = _gpu_encode(engine, pcm, mode)
        bad = [(s, f) for s in range(len(pcm)) for f in range(3) if not np.array_equal(got[s, f], want[s, f])]
        assert not bad, "%s: frames differ: %s" % (kind, bad)
    # a negative-shift quantisation in the oracle is a coded coefficient with a negative shift: its block took the exact path
    assert negshift > 0, "no block of this content has a negative shift: the exact path was not exercised"


def test_transcode_packers_agree(engine):
    """ac3mi_transcode_batch of the bench's shape through both packers: the same frames."""
    import torch
    pkg = H.pkg()
    streams = [H.orc_encode(H.gen_pcm(1, 6, seed=900 + s, kind=("tones", "music", "bursts", "noise")[s % 4])) for s in range(32)]
    frames_t = torch.from_numpy(np.stack(streams)).cuda()
    dec = pkg.DecodeDesc(flags=7 | 16 | 32, level=1.0, bias=384.0, dynrng=1, acmod=7, lfeon=1, frame_bytes=streams[0].shape[1])
    enc = pkg.EncodeDesc(48000, 384000, 6)
    outs = []
    for mode in (1, 2):
        engine.set_encode_mode(mode)
        try:
            delay = torch.zeros((32, 6, 128), dtype=torch.float32, device="cuda")
            lfsr = torch.ones((32,), dtype=torch.int16, device="cuda")
            last = torch.zeros((32, 6, 256), dtype=torch.int16, device="cuda")
            csnr = torch.full((32,), 40, dtype=torch.int32, device="cuda")
            out, status = engine.transcode_batch(dec, enc, frames_t, delay, lfsr, H.CHMAP6, last, csnr)
            engine.sync()
        finally:
            engine.set_encode_mode(0)
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])
