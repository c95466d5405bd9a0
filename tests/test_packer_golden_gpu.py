"""GPU: the encoder's bitstreams in the configurations the oracle does not restate - channel coupling (begf 0 and 3, with and
without a limited bandwidth), audio bandwidth, 2/0 rematrixing - and the bench's transcode shape, through both packers,
against frames recorded from the packer before its single-form quantiser (tests/golden/packer_frames.npz).

The packer's mantissa passes (csrc/enc_mant.h) are shared by every configuration, so a coupled or band-limited frame must
not change by a byte when the quantiser is rewritten: the coupling pass is the one whose uncoded bins (below cplstrtmant)
sit BELOW its coded ones within a lane.  Coupling tests elsewhere check side information, decodability and energies; these
check the mantissa bytes.  The golden file is regenerated only on purpose: `record()` below, on a GPU, with the build whose
output is the reference."""
import os

import numpy as np
import pytest

from tests import _harness as H

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "packer_frames.npz")

# name -> (nch, bitrate, kind, packer mode, coupling (mode, begf), bandwidth (mode, chbwcod), rematrix, transcode)
CASES = {
    "cpl0_51": (6, 384000, "music", 1, (1, 0), (0, 50), 0, False),
    "cpl3_51": (6, 384000, "noise", 1, (1, 3), (0, 50), 0, False),
    "cpl3_51_bursts": (6, 384000, "bursts", 1, (1, 3), (0, 50), 0, False),
    "cpl0_51_bw": (6, 384000, "music", 1, (1, 0), (1, 30), 0, False),
    "cpl0_20_remat": (2, 192000, "music", 1, (1, 0), (0, 50), 1, False),
    "bw30_51_f": (6, 384000, "music", 1, (0, 0), (1, 30), 0, False),
    "bw30_51_b": (6, 384000, "music", 2, (0, 0), (1, 30), 0, False),
    "remat_20_f": (2, 192000, "tones", 1, (0, 0), (0, 50), 1, False),
    "remat_20_b": (2, 192000, "tones", 2, (0, 0), (0, 50), 1, False),
    "transcode_51_f": (6, 384000, "music", 1, (0, 0), (0, 50), 0, True),
    "transcode_51_b": (6, 384000, "bursts", 2, (0, 0), (0, 50), 0, True),
    "transcode_cpl3_51": (6, 384000, "noise", 1, (1, 3), (0, 50), 0, True),
}
S, F = 4, 2


def run_case(engine, name):
    import torch
    pkg = H.pkg()
    nch, bitrate, kind, mode, cpl, bw, remat, transcode = CASES[name]
    chmap = H.CHMAP6 if nch == 6 else tuple(range(8))
    seed = 1000 + 17 * sorted(CASES).index(name)
    pcm = [H.gen_pcm(F, nch, seed=seed + s, kind=kind) for s in range(S)]
    enc = pkg.EncodeDesc(48000, bitrate, nch)
    last = torch.zeros((S, nch, 256), dtype=torch.int16, device="cuda")
    csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
    engine.set_encode_mode(mode)
    engine.set_encode_coupling(*cpl)
    engine.set_encode_bandwidth(*bw)
    engine.set_encode_rematrix(remat)
    try:
        if transcode:
            streams = np.stack([H.orc_encode(p) for p in pcm])
            frames = torch.from_numpy(streams).cuda()
            dec = pkg.DecodeDesc(flags=7 | 16 | 32, level=1.0, bias=384.0, dynrng=1, acmod=7, lfeon=1, frame_bytes=streams.shape[2])
            delay = torch.zeros((S, 6, 128), dtype=torch.float32, device="cuda")
            lfsr = torch.ones((S,), dtype=torch.int16, device="cuda")
            out, _ = engine.transcode_batch(dec, enc, frames, delay, lfsr, chmap[:nch], last, csnr)
        else:
            x = torch.from_numpy(np.stack(pcm).reshape(S, F, 1536, nch)).cuda()
            out = engine.encode_batch(enc, x, chmap[:nch], last, csnr)
        engine.sync()
    finally:
        engine.set_encode_mode(0)
        engine.set_encode_coupling(0, 0)
        engine.set_encode_bandwidth(0, 50)
        engine.set_encode_rematrix(0)
    return out.cpu().numpy()[:, :, :enc.frame_bytes()].copy()


def record(path):
    """Writes the golden frames of every case with the library the engine loads (AC3MI_LIB selects a build)."""
    pkg = H.pkg()
    eng = pkg.Engine(0)
    np.savez_compressed(path, **{name: run_case(eng, name) for name in CASES})
    eng.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_frames_equal_the_recorded_ones(engine, name):
    want = np.load(GOLDEN)[name]
    got = run_case(engine, name)
    assert got.shape == want.shape
    bad = [(s, f, int((got[s, f] != want[s, f]).sum())) for s in range(S) for f in range(F) if not np.array_equal(got[s, f], want[s, f])]
    assert not bad, "frames differ (stream, frame, bytes): %s" % bad
