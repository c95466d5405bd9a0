"""GPU: enc_packf_kernel<true> forms a 5.1 frame's side information from images (csrc/enc_syntax.h: syn_block_images_51 - a
prefix and a suffix per block that three lanes OR into the frame, one bit offset per exponent row) instead of field by field
through the accumulator.  Every frame must be the encoder oracle's byte for byte, and the same call under
ac3mi_set_fixed_shape 0 - the generic enc_packf_kernel, which writes through syn_block - must give the same bytes; the launch
log says which of the two ran.

Shapes: 1, 7 and 9 one-frame 5.1 streams at 384 kbps (fewer than the eight XCD slots, and one more) and 3 x 3 frames (the
tabulating search in front).  Contents, by the exponent sets a frame sends (read from the oracle's frames by
tests/ac3_syntax.parse_frame, asserted):
  stationary      the harness's tones: block 0's six sets alone - five empty prefixes' worth of reuse
  every block new band-hopping noise (hopping): all 36 sets, the LFE's among them - the longest prefixes, every row offset
  second generation  bursts and music encoded, decoded by the engine and encoded again: a mix of new and reused sets
and three calls that move the frame's bit position in ways a closed form could miss: a starved rate whose every search fails
(test_encode_gpu.test_starved_bit_rate_is_survivable's content; the mantissas overrun the frame, so both routes are compared
with each other - the oracle's bytes for it are pinned in tests/test_encode_ref_gpu.py), the merged-code marker moved to 26
(dropped mantissa fields), and block switching (the blksw flags of the prefix; a tool, so no oracle: the generic route)."""
import ctypes
import os

import numpy as np
import pytest

from tests import _harness as H
from tests import _tools as T
from tests import ac3_syntax as A
from tests import variant_matrix as V

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (7, 1), (9, 1), (3, 3)]
# seeds whose hopping frames send 36 sets from a new stream's state (block 1 of a first frame is the one that may fall short:
# its window holds one segment's bands more than block 0's, not two); the test asserts it
HOP_SEEDS = {1: (1000, 1001, 1002, 1006, 1007, 1008, 1009, 1013, 1015), 3: (2002, 2004, 2005)}
_SEG = ((0,), (1, 2), (3,))


def hopping(F, seed, amp=14000):
    """[F*1536][6] s16: per channel four noise bands, gated per 256-sample segment in the cycle {A}, {B, C}, {D} (the bands
    rotated by the channel): the window of every block holds another set of bands than the block before it, two bands or
    more apart - over 1000 in summed exponent differences, a new set in every block (ac3enc.cpp's strategy rule)"""
    rng = np.random.default_rng(seed)
    n = F * 1536
    out = np.zeros((n, 6))
    k = np.ones(32) / 32
    for c in range(6):
        for band in range(4):
            X = np.fft.rfft(rng.standard_normal(n))
            m = np.zeros(X.size)
            lo = X.size * band // 4
            m[lo + 1:lo + X.size // 4] = 1
            x = np.fft.irfft(X * m, n)
            x *= amp / np.abs(x).max()
            on = np.array([((band - c) % 4) in _SEG[s % 3] for s in range(n // 256)], np.float64).repeat(256)
            out[:, c] += x * np.convolve(np.convolve(on, k, mode="same"), k, mode="same")
    return np.clip(np.round(out), -32768, 32767).astype(np.int16)


def new_sets(frame):
    return sum(1 for B in A.parse_frame(frame).blocks for v in B.expstr.values() if v)


def oracle(pcm, rate=384000):
    return np.stack([H.orc_encode(p, 6, rate) for p in pcm])


def both_routes(engine, pcm, rate=384000, **tools):
    """the call with one wavefront per frame packing, fixed shape on and off -> (frames of the first, of the second); the
    launch log: enc_packf_kernel<true> and the generic name"""
    got = {}
    try:
        for fixed in (1, 0):
            engine.set_fixed_shape(fixed)
            with V.tap(engine) as names:
                got[fixed] = T.encode(engine, pcm, rate=rate, pack=1, **tools)
            packers = [n for n in names if n.startswith("enc_pack")]
            assert packers == [V.packf(fx=fixed)], (fixed, names)
    finally:
        engine.set_fixed_shape(1)
    return got[1], got[0]


def differing(a, b):
    return [(s, f, int(np.nonzero(a[s, f] != b[s, f])[0][0])) for s in range(a.shape[0]) for f in range(a.shape[1]) if not np.array_equal(a[s, f], b[s, f])]


_PCM = {}


def source(kind, F):
    """[9 or 3][F*1536][6] s16 of a first-generation content, and (computed once, shared) the oracle's frames for it"""
    if (kind, F) not in _PCM:
        S = 9 if F == 1 else 3
        if kind == "stationary":
            pcm = np.stack([H.gen_pcm(F, 6, seed=6100 + s, kind="tones") for s in range(S)])
        elif kind == "every block new":
            pcm = np.stack([hopping(F, seed) for seed in HOP_SEEDS[F]])
        else:
            pcm = np.stack([H.gen_pcm(F, 6, seed=6200 + s, kind=("bursts", "music")[s % 2]) for s in range(S)])
        _PCM[(kind, F)] = (pcm, oracle(pcm))
    return _PCM[(kind, F)]


@pytest.mark.parametrize("S,F", SHAPES)
@pytest.mark.parametrize("kind", ["stationary", "every block new"])
def test_first_generation(engine, kind, S, F):
    pcm, want = source(kind, F)
    pcm, want = pcm[:S], want[:S]
    sets = [new_sets(want[s, f]) for s in range(S) for f in range(F)]
    assert set(sets) == ({6} if kind == "stationary" else {36}), sets
    fx, generic = both_routes(engine, pcm)
    assert not differing(fx, want), "fixed shape against the oracle (stream, frame, first byte): %r" % differing(fx, want)
    assert not differing(generic, want), "generic against the oracle: %r" % differing(generic, want)


@pytest.mark.parametrize("S,F", SHAPES)
def test_second_generation(engine, S, F):
    """the engine's own decoded output encoded again: frames with some rows new and some reused in most blocks"""
    src, _ = source("mix", F)
    src = src[:S]
    first = T.encode(engine, src, pack=1)
    dec, status, _ = T.decode(engine, first, 7, 1)
    assert dec.shape == (S, F, 6, 6, 256) and (status & 0x1ff).max() == 0
    pcm = np.clip(np.round(dec.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    pcm = np.ascontiguousarray(pcm.transpose(0, 1, 2, 4, 3).reshape(S, F * 1536, 6))
    want = oracle(pcm)
    sets = [new_sets(want[s, f]) for s in range(S) for f in range(F)]
    assert any(6 < n < 36 for n in sets), sets
    fx, generic = both_routes(engine, pcm)
    assert not differing(fx, want), "fixed shape against the oracle (stream, frame, first byte): %r" % differing(fx, want)
    assert not differing(generic, want), "generic against the oracle: %r" % differing(generic, want)


def test_failed_search(engine):
    """6 channels of noise at 64 kbps: no offset fits, the header repeats the start value's offsets and the blocks run far
    beyond the frame's 256 bytes - side information of the later blocks lands in the headroom or is dropped"""
    pcm = np.stack([H.gen_pcm(1, 6, seed=880 + s, kind="noise") for s in range(7)])
    fx, generic = both_routes(engine, pcm, rate=64000)
    assert fx.shape == (7, 1, 256) and (fx[:, :, 0] == 0x0b).all() and (fx[:, :, 1] == 0x77).all()
    assert not differing(fx, generic), "fixed shape against generic (stream, frame, first byte): %r" % differing(fx, generic)


def test_marker_26(engine):
    """grouped codes equal to 26 are not written (test_encode_gpu.test_grouped_code_equal_to_the_merged_marker_is_not_written):
    every block's mantissas end elsewhere than their counts say, and the next block's images go where they end"""
    L = H.orc()
    L.orc_ac3enc_set_marker.argtypes = [ctypes.c_int]
    pcm = np.stack([H.gen_pcm(1, 6, seed=40 + s, kind="noise") for s in range(7)])
    plain = oracle(pcm)
    L.orc_ac3enc_set_marker(26)
    os.environ["AC3MI_ENC_MARKER"] = "26"
    try:
        want = oracle(pcm)
        fx, generic = both_routes(engine, pcm)
    finally:
        L.orc_ac3enc_set_marker(128)
        del os.environ["AC3MI_ENC_MARKER"]
    assert len(differing(want, plain)) == 7, "this content has no code equal to 26 in some frame"
    assert not differing(fx, want), "fixed shape against the oracle (stream, frame, first byte): %r" % differing(fx, want)
    assert not differing(generic, want), "generic against the oracle: %r" % differing(generic, want)


def test_block_switching(engine):
    """blksw flags in the prefix image (ac3mi_set_encode_block_switch: a burst per frame in channel 0)"""
    pcm = T.content("attack", 6, 7, 1, seed=6300)
    fx, generic = both_routes(engine, pcm, bsw=1)
    flags = [B.fields["blksw%d" % ch] for s in range(7) for B in A.parse_frame(fx[s, 0]).blocks for ch in range(5)]
    assert any(flags) and not all(flags), "no block switched"
    assert not differing(fx, generic), "fixed shape against generic (stream, frame, first byte): %r" % differing(fx, generic)
