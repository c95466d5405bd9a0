"""GPU: the window sweep of the encoder's SNR-offset search (enc_search_kernel<1>, csrc/snr_window.h) against the oracle's
spare-bit curves.  The debug tap ac3mi_debug_search_curve hands out, per frame, the spare bits and the ceiling sixths of every
offset the search costed; each such entry must equal the oracle's count at that offset (orc_ac3enc_set_spare_curve /
_set_extra_curve) exactly, the frames must equal the oracle's byte for byte and the stream state must end at the oracle's
offsets - on fresh bench-like audio (cold, then warm in a second call), on its transcode, at the extremes of the offset
range, on other layouts and rates, on a stream of four frames.  The fixed-shape search gives the same frames as the generic
one, and coupled frames - which the oracle does not restate - equal frames recorded from the three-offset search
(tests/golden/search_window_cpl.npz: written by `record()` below on an MI355X with AC3MI_LIB naming a library built from commit
67daf7e, "Encoder: state the frame's side-information syntax once", the last commit whose PART 1 search costs three offsets a
sweep)."""
import ctypes
import os

import numpy as np
import pytest

from tests import _harness as H

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_window_cpl.npz")
UNCOSTED = -2 ** 31


def bench_like_pcm(S, F, seed):
    """the benchmark's kind of audio (profiles/search_sim.py curves): a sine per channel, noise, level steps of 30 dB"""
    import torch
    g = torch.Generator().manual_seed(seed)
    n = 1536 * F
    t = torch.arange(n, dtype=torch.float32)
    ph = torch.rand((S, 1, 6), generator=g) * 6.28
    fr = 0.01 * torch.arange(1, 7, dtype=torch.float32)
    pcm = 8000.0 * torch.sin(ph + fr * t[None, :, None]) + (torch.rand((S, n, 6), generator=g) - 0.5) * 4096
    env = torch.where(torch.rand((S, 3 * F, 1, 6), generator=g) < 0.5, 1.0, 1.0 / 32)
    pcm = (pcm.reshape(S, 3 * F, 512, 6) * env).reshape(S, n, 6)
    return pcm.round().clamp(-32768, 32767).to(torch.int16).numpy()


def oracle(pcm, nch, bitrate):
    """pcm [S][F * 1536][nch] -> frames [S][F][fb], spare bits and sixths [S][F][1024], offsets after each frame [S][F][2]"""
    L = H.orc()
    L.orc_ac3enc_set_spare_curve.argtypes = [ctypes.c_void_p]
    L.orc_ac3enc_set_extra_curve.argtypes = [ctypes.c_void_p]
    S, F = pcm.shape[0], pcm.shape[1] // 1536
    cm = (ctypes.c_uint8 * 8)(*(H.CHMAP6 if nch == 6 else tuple(range(8))))
    spare, extra = np.zeros(1024, np.int32), np.zeros(1024, np.int32)
    fb = H.ci()
    out = None
    curves, sixths, snr = np.zeros((S, F, 1024), np.int32), np.zeros((S, F, 1024), np.int32), np.zeros((S, F, 2), np.int32)
    L.orc_ac3enc_set_spare_curve(spare.ctypes.data)
    L.orc_ac3enc_set_extra_curve(extra.ctypes.data)
    try:
        for s in range(S):
            h = L.orc_ac3enc_init(48000, bitrate, nch, ctypes.byref(fb))
            assert h
            if out is None:
                out = np.zeros((S, F, fb.value), np.uint8)
            x = np.ascontiguousarray(pcm[s])
            for f in range(F):
                assert L.orc_ac3enc_frame(h, H.P(out[s, f], H.u8p), ctypes.cast(x.ctypes.data + f * 1536 * nch * 2, H.i16p), cm) == fb.value
                st, sh = np.zeros((6, 6), np.uint8), np.zeros((6, 6), np.int8)
                c, fs = H.ci(), H.ci()
                L.orc_ac3enc_get_misc(h, H.P(st, H.u8p), H.P(sh, H.i8p), ctypes.byref(c), ctypes.byref(fs))
                curves[s, f], sixths[s, f], snr[s, f] = spare, extra, (c.value, fs.value)
            L.orc_ac3enc_free(h)
    finally:
        L.orc_ac3enc_set_spare_curve(None)
        L.orc_ac3enc_set_extra_curve(None)
    return out, curves, sixths, snr


class Tapped:
    """encode / transcode calls on `engine` with the search's tap set"""

    def __init__(self, engine, S, F):
        import torch
        self.engine = engine
        self.tap = torch.full((S, F, 1024, 2), UNCOSTED, dtype=torch.int32, device="cuda")

    def __enter__(self):
        self.engine.debug_search_curve(self.tap)
        return self

    def __exit__(self, *exc):
        self.engine.sync()
        self.engine.debug_search_curve(None)

    def curve(self):
        return self.tap.cpu().numpy()


def check_tap(tap, curves, sixths, every_frame=True):
    """every costed entry is the oracle's; a frame whose search ran cost whole windows"""
    costed = tap[..., 0] != UNCOSTED
    n = costed.sum(axis=-1)
    if every_frame:
        assert (n >= 16).all(), n.tolist()
    assert costed.any()
    bad = costed & ((tap[..., 0] != curves) | (tap[..., 1] != sixths))
    where = np.argwhere(bad)
    assert not bad.any(), [(tuple(int(v) for v in w), tap[tuple(w)].tolist(), int(curves[tuple(w)]), int(sixths[tuple(w)])) for w in where[:5]]
    return n


def encode(engine, pcm, nch, bitrate, last=None, csnr=None):
    import torch
    pkg = H.pkg()
    S, F = pcm.shape[0], pcm.shape[1] // 1536
    desc = pkg.EncodeDesc(48000, bitrate, nch)
    chmap = (H.CHMAP6 if nch == 6 else tuple(range(8)))[:nch]
    last = torch.zeros((S, nch, 256), dtype=torch.int16, device="cuda") if last is None else last
    csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda") if csnr is None else csnr
    out = engine.encode_batch(desc, torch.from_numpy(pcm.reshape(S, F, 1536, nch)).cuda(), chmap, last, csnr)
    engine.sync()
    return out.cpu().numpy()[:, :, :desc.frame_bytes()], last, csnr


def state_offsets(csnr):
    v = csnr.cpu().numpy()
    return np.stack([v & 0xff, (v >> 8) & 15], axis=1)


@pytest.fixture(scope="module")
def fresh():
    """48 streams of two frames of bench-like audio and what the oracle makes of them"""
    pcm = bench_like_pcm(48, 2, seed=99)
    return (pcm,) + oracle(pcm, 6, 384000)


def test_fresh_streams_cold_then_warm(engine, fresh):
    """one-frame calls, as the benchmark's: frame 0 from the cold state, frame 1 from the state frame 0 left"""
    pcm, want, curves, sixths, snr = fresh
    S = pcm.shape[0]
    with Tapped(engine, S, 1) as t0:
        got0, last, csnr = encode(engine, pcm[:, :1536], 6, 384000)
    n0 = check_tap(t0.curve(), curves[:, :1], sixths[:, :1])
    assert np.array_equal(got0, want[:, :1])
    assert np.array_equal(state_offsets(csnr), snr[:, 0])
    with Tapped(engine, S, 1) as t1:
        got1, last, csnr = encode(engine, pcm[:, 1536:], 6, 384000, last, csnr)
    n1 = check_tap(t1.curve(), curves[:, 1:], sixths[:, 1:])
    assert np.array_equal(got1, want[:, 1:])
    assert np.array_equal(state_offsets(csnr), snr[:, 1])
    # sixteen offsets a sweep; the rule's bounded fallback holds on the device as in the simulator
    assert n0.max() <= 12 * 16 and n1.max() <= 12 * 16
    for name, n in (("cold", n0), ("warm", n1)):
        print("fresh, %s: costed offsets / 16 per frame: mean %.2f, histogram %s" % (name, n.mean() / 16.0, np.bincount((n.reshape(-1) + 15) // 16).tolist()))


def test_fixed_shape_and_generic_search_agree(engine, fresh):
    pcm, want, curves, sixths, snr = fresh
    outs = []
    for on in (1, 0):
        engine.set_fixed_shape(on)
        try:
            got, last, csnr = encode(engine, pcm[:, :1536], 6, 384000)
        finally:
            engine.set_fixed_shape(1)
        outs.append((got, state_offsets(csnr)))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert np.array_equal(outs[0][0], want[:, :1]) and np.array_equal(outs[0][1], snr[:, 0])


@pytest.mark.parametrize("decode_mode", [4, 0])
def test_transcode_with_the_sources_offsets_as_hint(engine, fresh, decode_mode):
    """the oracle's frames decoded and re-encoded by ac3mi_transcode_batch: the curves are the oracle's on the s16 audio the
    engine's own decoder hands its encoder (decode_batch + convert_s16_batch: a float32 ulp at bias 384 is an s16 step).
    The hint - the source frame's offsets - reaches the search from the split front end's descriptors alone: decode mode 4
    takes that front end at any batch size, and the first window must then start five steps below the source's offsets
    (win_first_lo).  Mode 0 at 48 streams takes the fused decoder: the same call without a hint, first window at g = 176."""
    import torch
    pkg = H.pkg()
    pcm, first_gen, _, _, src_snr = fresh
    S = pcm.shape[0]
    engine.set_decode_mode(decode_mode)
    try:
        _transcode_case(engine, pkg, torch, S, first_gen, src_snr, decode_mode)
    finally:
        engine.set_decode_mode(0)


def _transcode_case(engine, pkg, torch, S, first_gen, src_snr, decode_mode):
    src = np.ascontiguousarray(first_gen[:, :1])
    frames_t = torch.from_numpy(src).cuda()
    dec = pkg.DecodeDesc(flags=7 | 16 | 32, level=1.0, bias=384.0, dynrng=1, acmod=7, lfeon=1, frame_bytes=src.shape[2])
    enc = pkg.EncodeDesc(48000, 384000, 6)

    def states():
        return (torch.zeros((S, 6, 128), dtype=torch.float32, device="cuda"), torch.ones((S,), dtype=torch.int16, device="cuda"),
                torch.zeros((S, 6, 256), dtype=torch.int16, device="cuda"), torch.full((S,), 40, dtype=torch.int32, device="cuda"))

    delay, lfsr, last, csnr = states()
    planes, status = engine.decode_batch(dec, frames_t, delay, lfsr)
    s16 = torch.empty((S * 6, 256, 6), dtype=torch.int16, device="cuda")
    engine.sync()
    _, oflags = engine.decode_planes(dec)
    engine._check(engine.lib.ac3mi_convert_s16_batch(ctypes.c_void_p(engine.ctx), ctypes.c_void_p(planes.data_ptr()),
                                                     ctypes.c_void_p(s16.data_ptr()), oflags, ctypes.c_size_t(S * 6)))
    engine.sync()
    want, curves, sixths, snr = oracle(s16.cpu().numpy().reshape(S, 1536, 6), 6, 384000)
    delay, lfsr, last, csnr = states()
    with Tapped(engine, S, 1) as t:
        out, status = engine.transcode_batch(dec, enc, frames_t, delay, lfsr, H.CHMAP6, last, csnr)
    tap = t.curve()
    check_tap(tap, curves, sixths)
    assert np.array_equal(out.cpu().numpy()[:, :, :want.shape[2]], want)
    assert np.array_equal(state_offsets(csnr), snr[:, 0])
    # where the first window began: the lowest costed offset is no higher, and it is costed
    src_g = 16 * src_snr[:, 0, 0] + src_snr[:, 0, 1]
    first_lo = np.clip(src_g - 5, 0, 1008) if decode_mode == 4 else np.full(S, 176)
    costed = tap[:, 0, :, 0] != UNCOSTED
    assert costed[np.arange(S), first_lo].all(), (decode_mode, first_lo.tolist())
    # a frame done in one sweep costed exactly its first window; most are
    one = costed.sum(axis=1) == 16
    assert one.sum() > S // 2, int(one.sum())
    for s_ in np.nonzero(one)[0]:
        assert np.array_equal(np.nonzero(costed[s_])[0], np.arange(first_lo[s_], first_lo[s_] + 16)), (decode_mode, int(s_), int(first_lo[s_]))
    if decode_mode == 4:
        assert (first_lo != 176).any()              # (the hinted windows are not the cold one by chance)
    print("transcode, decode mode %d: costed offsets / 16 per frame: mean %.2f, histogram %s" % (
        decode_mode, costed.sum(axis=1).mean() / 16.0, np.bincount((costed.sum(axis=1) + 15) // 16).tolist()))
    # and without the tap, through the kernels a transcode of this shape takes by itself
    delay, lfsr, last, csnr = states()
    out2, _ = engine.transcode_batch(dec, enc, frames_t, delay, lfsr, H.CHMAP6, last, csnr)
    engine.sync()
    assert torch.equal(out2.cpu(), out.cpu()) and np.array_equal(state_offsets(csnr), snr[:, 0])


@pytest.mark.parametrize("kind,nch,bitrate", [("silence", 6, 384000), ("noise", 6, 224000), ("tones", 1, 64000), ("music", 6, 640000)])
def test_the_ends_of_the_range_and_other_shapes(engine, kind, nch, bitrate):
    """digital silence lands at the top (g = 1023), full-scale noise at 224 kbps near 0 or on the reference's failure path"""
    S = 8
    pcm = np.stack([H.gen_pcm(1, nch, seed=900 + 13 * s, kind=kind) for s in range(S)])
    want, curves, sixths, snr = oracle(pcm, nch, bitrate)
    with Tapped(engine, S, 1) as t:
        got, last, csnr = encode(engine, pcm, nch, bitrate)
    check_tap(t.curve(), curves, sixths)
    assert np.array_equal(got, want), "frames differ in %d bytes" % int((got != want).sum())
    assert np.array_equal(state_offsets(csnr), snr[:, 0])
    if kind == "silence":
        assert (16 * snr[:, 0, 0] + snr[:, 0, 1] == 1023).all()
    got2, _, csnr2 = encode(engine, pcm, nch, bitrate)              # the untapped call
    assert np.array_equal(got2, want) and np.array_equal(state_offsets(csnr2), snr[:, 0])


def test_a_stream_of_four_frames(engine):
    """frames 1..3 start warm, from the offsets of the frame before; no hint.  One long stream goes through PART 3's
    tabulation first, which may answer every question of a frame before the replay costs anything: every_frame is off, and this
    case checks the replay's bytes, state and whatever it does cost.  The warm first window itself is checked, frame by frame,
    by the second one-frame call of test_fresh_streams_cold_then_warm."""
    pcm = bench_like_pcm(1, 4, seed=7)
    want, curves, sixths, snr = oracle(pcm, 6, 384000)
    with Tapped(engine, 1, 4) as t:
        got, last, csnr = encode(engine, pcm, 6, 384000)
    check_tap(t.curve(), curves, sixths, every_frame=False)
    assert np.array_equal(got, want)
    assert np.array_equal(state_offsets(csnr), snr[:, 3])


# ---- coupled frames: recorded from the three-offset search ----
CPL_CASES = {"begf0_music": (0, "music", 1), "begf3_noise": (3, "noise", 1), "begf0_bursts_2f": (0, "bursts", 2), "begf3_tones_2f": (3, "tones", 2)}


def run_cpl(engine, name):
    begf, kind, F = CPL_CASES[name]
    pcm = np.stack([H.gen_pcm(F, 6, seed=1300 + 11 * s + begf, kind=kind) for s in range(4)])
    engine.set_encode_coupling(1, begf)
    try:
        got, last, csnr = encode(engine, pcm, 6, 384000)
    finally:
        engine.set_encode_coupling(0, 0)
    return got.copy(), state_offsets(csnr)


def record(path):
    """Writes the golden frames with the library the engine loads (AC3MI_LIB selects a build)."""
    eng = H.pkg().Engine(0)
    data = {}
    for name in CPL_CASES:
        data[name], data[name + "_state"] = run_cpl(eng, name)
    np.savez_compressed(path, **data)
    eng.close()


@pytest.mark.parametrize("name", sorted(CPL_CASES))
def test_coupled_frames_equal_the_recorded_ones(engine, name):
    gold = np.load(GOLDEN)
    got, state = run_cpl(engine, name)
    assert np.array_equal(got, gold[name]), "frames differ in %d bytes" % int((got != gold[name]).sum())
    assert np.array_equal(state, gold[name + "_state"])
