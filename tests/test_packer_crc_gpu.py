"""GPU: the two CRC words the packers store (csrc/crc_lanes.h: both regions in one lane pass, one multiplication per lane, a table
per frame size kept by the context) at the frame sizes where the rule can go wrong - not the workload's alone:

    48 kHz / 32 kbps mono       64 words: most lanes sum nothing but padding in front of their region
    44.1 kHz / 384 kbps 5.1     835 words, odd: both region ends are only halfword-aligned
    32 kHz / 640 kbps 5.1       1 920 words: the largest chunk (60 bytes a lane)
    24 kHz / 48 kbps mono       a half-rate configuration (bsid 9)
    48 kHz / 384 kbps 5.1       the fixed-shape kernel
    24 kHz / 48 kbps, 3 channels    frames whose search fails (ENC/ac3enc.cpp:921-933, tests/test_encode_gpu.py)
    48 kHz / 64 kbps stereo     frames whose bit budget overshoots into the crc2 field (:1609-1613; found as tests/test_crc_gpu.py does)

Eight streams each through both packers (ac3mi_set_encode_mode 1: enc_packf_kernel, 2: enc_packb_kernel).  Every frame must equal
the encoder oracle's byte for byte, and both regions must sum to zero by the definition (tests/crc_model.py) - the words cover
whatever the frame holds.  All of it runs twice in ONE fresh context, so every configuration meets another frame size before it
comes again: the second pass, served from the context's table cache, must equal the first."""
import ctypes

import numpy as np
import pytest

from tests import _harness as H
from tests import crc_model as M
from tests import variant_matrix as V

pytestmark = pytest.mark.gpu

# name -> (channels, bit rate, sample rate, frame words, frames per stream, kinds)
CASES = {
    "mono_64w": (1, 32000, 48000, 64, 2, ("tones", "music", "noise", "bursts")),
    "51_835w": (6, 384000, 44100, 835, 2, ("tones", "music", "noise", "bursts")),
    "51_1920w": (6, 640000, 32000, 1920, 2, ("tones", "music", "noise", "strobe")),
    "mono_halfrate": (1, 48000, 24000, 192, 2, ("tones", "music", "noise", "quiet")),
    "51_768w": (6, 384000, 48000, 768, 2, ("tones", "music", "noise", "bursts")),
    "3ch_search_fails": (3, 48000, 24000, 192, 4, None),
    "stereo_overshoot": (2, 64000, 48000, 128, 2, ("noise",)),
}
S = 8


def _pcm(name):
    nch, _, _, _, F, kinds = CASES[name]
    if kinds is None:       # tests/test_encode_gpu.py, test_failed_search_follows_the_reference: streams 0 and 3 hold a frame whose search fails
        return [H.gen_pcm(F, nch, seed=101000 + 25 * 7 + (s % 4), kind=("music", "tones", "tones", "music")[s % 4]) for s in range(S)]
    return [H.gen_pcm(F, nch, seed=7100 + s, kind=kinds[s % len(kinds)]) for s in range(S)]


def _chmap(nch):
    return H.CHMAP6 if nch == 6 else tuple(range(8))


def _oracle(name):
    nch, bitrate, freq, fs, F, _ = CASES[name]
    L = H.orc()
    cm = (ctypes.c_uint8 * 8)(*_chmap(nch))
    want = np.zeros((S, F, 2 * fs), np.uint8)
    for s, p in enumerate(_pcm(name)):
        src = np.ascontiguousarray(p.reshape(-1))
        assert L.orc_ac3enc_encode_frames(freq, bitrate, nch, H.P(src, H.i16p), F, cm, H.P(want[s], H.u8p)) == 0
    return want


def _encode(eng, name, mode):
    import torch
    pkg = H.pkg()
    nch, bitrate, freq, fs, F, _ = CASES[name]
    desc = pkg.EncodeDesc(freq, bitrate, nch)
    assert desc.frame_bytes() == 2 * fs
    x = torch.from_numpy(np.stack(_pcm(name)).reshape(S, F, 1536, nch)).cuda()
    last = torch.zeros((S, nch, 256), dtype=torch.int16, device="cuda")
    csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
    eng.set_encode_mode(mode)
    try:
        with V.tap(eng) as log:
            out = eng.encode_batch(desc, x, _chmap(nch)[:nch], last, csnr)
            eng.sync()
    finally:
        eng.set_encode_mode(0)
    assert ("enc_packf_kernel" if mode == 1 else "enc_packb_kernel") in V.families(log), (name, mode, log)
    return out.cpu().numpy()[:, :, :2 * fs].copy()


@pytest.fixture(scope="module")
def passes():
    """[pass][(name, mode)] -> frames: every configuration and packer, twice over, in one context of its own"""
    eng = H.pkg().Engine(0)
    try:
        return [{(name, mode): _encode(eng, name, mode) for name in CASES for mode in (1, 2)} for _ in range(2)]
    finally:
        eng.close()


@pytest.fixture(scope="module")
def oracle_frames():
    return {name: _oracle(name) for name in CASES}


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", sorted(CASES))
def test_frames_equal_the_oracle_and_seal_both_regions(passes, oracle_frames, name, mode):
    want, got = oracle_frames[name], passes[0][(name, mode)]
    fs = CASES[name][3]
    assert got.shape == want.shape
    bad = [(s, f, int((got[s, f] != want[s, f]).sum())) for s in range(S) for f in range(got.shape[1]) if not np.array_equal(got[s, f], want[s, f])]
    assert not bad, "frames differ from the oracle (stream, frame, bytes): %s" % bad
    flat = got.reshape(-1, 2 * fs)
    assert all(M.frame_size(f[:6]) == 2 * fs for f in flat)
    v = M.verdicts(flat)
    assert not v.any(), "regions that do not sum to zero (frame, verdict): %s" % [(i, int(x)) for i, x in enumerate(v) if x]


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", sorted(CASES))
def test_second_pass_from_the_table_cache_equals_the_first(passes, name, mode):
    assert np.array_equal(passes[1][(name, mode)], passes[0][(name, mode)])


def test_the_quirk_cases_hold_what_their_names_say(oracle_frames):
    """frames whose crc2 field was written over by mantissas before the word went in; frames whose search failed"""
    from tests import ac3_syntax as A
    st = oracle_frames["stereo_overshoot"]
    fb = st.shape[2]
    over = sum(A.parse_frame(f).blocks[5].end > 8 * fb - A.TAIL_BITS for f in st.reshape(-1, fb))
    print("stereo frames whose bit budget overshoots: %d" % over)
    assert over >= 1
    # a frame whose search failed carries the mantissas of an allocation that does not fit: it runs over its end and no longer parses
    # (frame 3 of streams 0 and 4, frame 2 of streams 3 and 7: test_encode_gpu.test_failed_search_follows_the_reference)
    fl = oracle_frames["3ch_search_fails"]

    def parses(f):
        try:
            A.parse_frame(f)
            return True
        except A.SyntaxError_:
            return False
    broken = {(s, f) for s in range(S) for f in range(fl.shape[1]) if not parses(fl[s, f])}
    assert {(0, 3), (3, 2), (4, 3), (7, 2)} <= broken, broken
