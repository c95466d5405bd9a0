"""GPU: the BSI reader kernel (ac3mi_bsi_read_batch) against the host function, per-frame encoder metadata
(ac3mi_set_encode_metadata_frames) and the transcode that follows its source (ac3mi_set_encode_metadata_source 1) against
tests/bsi_model.py and against what ac3mi_set_encode_metadata - pinned by test_drc_gpu.py and drc_model - does for one word.
Batches of 8 to 16 streams of 1 to 3 frames."""
import ctypes
import importlib

import numpy as np
import pytest

from tests import _harness as H
from tests import _tools as T
from tests import ac3_syntax as A
from tests import bsi_model as M
from tests import packer

pytestmark = pytest.mark.gpu

ERR_ARG = -1


def _capi():
    return importlib.import_module(H.pkg().__name__ + ".capi")


def _restore(engine):
    engine.set_encode_metadata_frames(None)
    engine.set_encode_metadata_source(0)
    engine.set_encode_metadata()
    engine.set_encode_layout(0)
    engine.set_encode_mode(0)
    engine.set_decode_crc(0)
    engine.set_tile_frames(131072)
    engine._check(engine.lib.ac3mi_set_state_slots(ctypes.c_void_p(engine.ctx), None))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reader kernel

def test_reader_kernel_equals_host_function(engine):
    """a mixed batch - packer frames of several acmods and sizes, 44.1 kHz frames of both sizes, garbage, broken headers - on a
    stride that is no multiple of 16: every record is the host function's, frames longer than frame_bytes are not read, and
    the canary bytes behind the record array are intact"""
    import torch
    pkg = H.pkg()
    dt = _capi().bsi_info_dtype()
    rng = np.random.default_rng(77)
    frames = []
    for acmod, lfeon, kw in ((0, 1, dict(frmsizecod=20)), (1, 0, dict(frmsizecod=12)), (2, 0, dict(frmsizecod=16)), (3, 1, dict(frmsizecod=20)),
                             (5, 0, dict(frmsizecod=24)), (7, 1, dict(frmsizecod=24, bsid=9)), (2, 1, dict(fscod=1, frmsizecod=20)),
                             (2, 1, dict(fscod=1, frmsizecod=21)), (6, 0, dict(fscod=2, frmsizecod=22))):
        for opts in (0.0, 1.0):
            frames.append(packer.make_frame(rng, acmod, lfeon, features=dict(bsi_opts=opts), **kw))
    fb = max(len(f) for f in frames)
    stride = ((fb + 3) & ~3) + 4
    if stride % 16 == 0:
        stride += 4
    n = len(frames) + 6
    batch = np.zeros((n, stride), np.uint8)
    for i, f in enumerate(frames):
        batch[i, :len(f)] = f
    k = len(frames)
    batch[k] = rng.integers(0, 256, stride)                          # noise
    batch[k + 1] = 0xff
    batch[k + 2, :len(frames[0])] = frames[0]
    batch[k + 2, 0] = 0                                              # no sync word
    batch[k + 3, :len(frames[1])] = frames[1]
    batch[k + 3, 4] = (batch[k + 3, 4] & 0xc0) | 40                  # frmsizecod 40
    batch[k + 4, :len(frames[2])] = frames[2]
    batch[k + 4, 4] |= 0xc0                                          # fscod 3
    batch[k + 5, :len(frames[3])] = frames[3]
    batch[k + 5, 5] |= 0x60                                          # bsid >= 12

    def host(frame_bytes):
        out = np.zeros(n, dt)
        for i in range(n):
            size = pkg.syncinfo(batch[i])[0]
            out[i] = pkg.bsi_read(batch[i, :frame_bytes])
            if size > frame_bytes and out[i]["verdict"] != 0x80:
                out[i] = np.zeros((), dt)
                out[i]["verdict"] = 0x80
        return out

    d_frames = torch.from_numpy(batch).cuda()
    for frame_bytes in (fb, fb - 2, 400):
        big = torch.full((n + 2, dt.itemsize), 0xa5, dtype=torch.uint8, device="cuda")
        engine.bsi_read_batch(d_frames, frame_bytes, out=big[:n])
        engine.sync()
        got = big.cpu().numpy()
        assert (got[n:] == 0xa5).all(), "canary"
        got = got[:n].copy().view(dt)[:, 0]
        want = host(frame_bytes)
        assert np.array_equal(got, want), (frame_bytes, np.nonzero(got != want)[0][:8])
        if frame_bytes == fb:
            assert (got["verdict"][:k] == 0).all() and (got["verdict"][k + 1:] == 0x80).all()
            for i, f in enumerate(frames):
                assert int(got["block0_bit"][i]) == M.parse_head(f).header_bits
        else:
            assert 0 < np.count_nonzero(got["verdict"][:k] == 0x80) < k
    # bad arguments are refused before any launch
    lib, ctx = engine.lib, ctypes.c_void_p(engine.ctx)
    out = torch.zeros((n, dt.itemsize), dtype=torch.uint8, device="cuda")
    fp, op = ctypes.c_void_p(d_frames.data_ptr()), ctypes.c_void_p(out.data_ptr())
    for args in ((None, stride, fb, n, op), (fp, stride, fb, n, None), (fp, stride + 2, fb, n, op), (fp, fb - 8, fb, n, op),
                 (fp, stride, 7, n, op), (fp, 3844, 3841, n, op)):
        assert lib.ac3mi_bsi_read_batch(ctx, args[0], args[1], args[2], ctypes.c_size_t(args[3]), args[4]) == ERR_ARG
    assert lib.ac3mi_bsi_read_batch(ctx, fp, stride, fb, ctypes.c_size_t(0), op) == 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. / 3. a word per frame in the encoder

def _random_words(rng, S, F):
    """a different raw word for every frame, reserved codes among them, junk in bits 16-31"""
    w = rng.choice(1 << 16, S * F, replace=False).astype(np.int64)
    w[0] = M.pack_word(dialnorm=0, bsmod=7, cmixlev=3, surmixlev=3, dsurmod=3, copyrightb=1, origbs=0)
    w[1] &= ~31                                                        # dialnorm 0
    w[2] |= 0x3f00                                                     # all three mix codes reserved
    w |= rng.integers(0, 1 << 15, S * F).astype(np.int64) << 16
    return w.reshape(S, F)


def _words_tensor(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words).astype(np.uint32).view(np.int32)).cuda()


def _crc_ok(engine, frames):
    import torch
    S, F, fb = frames.shape
    buf = np.zeros((S * F, (fb + 3) & ~3), np.uint8)
    buf[:, :fb] = frames.reshape(S * F, fb)
    v = engine.crc_check_batch(torch.from_numpy(buf).cuda(), fb)
    engine.sync()
    return not v.cpu().numpy().any()


def _check_frames_carry_words(frames, plain, words, acmod):
    """each frame parses, carries sanitise(word) by its acmod, and equals the default-metadata frame in every bit outside the
    metadata fields and the two CRC words"""
    S, F, fb = frames.shape
    for s in range(S):
        for f in range(F):
            P = A.parse_frame(frames[s, f])
            assert P.acmod == acmod
            want = M.coded_fields(int(words[s, f]) & 0xffffffff, acmod)
            assert {k: P.fields[k] for k in want} == want, (s, f)
            assert set(M.sends(acmod)) <= set(want) and all(P.fields[k] < 3 for k in M.sends(acmod)) and P.fields["dialnorm"] != 0
            a, b = np.unpackbits(frames[s, f]), np.unpackbits(plain[s, f])
            free = np.zeros(a.size, bool)
            free[M.metadata_bits(P)] = True
            free[16:32] = True
            free[8 * fb - 16:] = True
            assert np.array_equal(a[~free], b[~free]), (s, f)


CONFIGS = {"1/0": dict(nch=1, acmod=1, kw={}),
           "2/0": dict(nch=2, acmod=2, kw={}),
           "2/0 coupled": dict(nch=2, acmod=2, kw=dict(cpl=(1, 2))),
           "3/2+LFE": dict(nch=6, acmod=7, kw={}),
           "dual mono": dict(nch=2, acmod=0, kw=dict(layout=(1, 0, 0)))}


@pytest.mark.parametrize("pack", [1, 2])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_per_frame_words_without_drc(engine, config, pack):
    c = CONFIGS[config]
    S, F = 8, 3
    pcm = T.content("music", c["nch"], S, F, seed=300 + c["nch"])
    words = _random_words(np.random.default_rng(5 + pack), S, F)
    try:
        plain = T.encode(engine, pcm, pack=pack, **c["kw"])
        engine.set_encode_metadata_frames(_words_tensor(words))
        got = T.encode(engine, pcm, pack=pack, **c["kw"])
        assert _crc_ok(engine, got)
        _check_frames_carry_words(got, plain, words, c["acmod"])
        if "cpl" in c["kw"]:
            assert any(T.coupling_view(f, c["nch"])[0] for f in got.reshape(-1, got.shape[2])), "no frame coupled"
        # ac3mi_set_encode_metadata's own word is not read while the array is set
        assert np.array_equal(T.encode(engine, pcm, pack=pack, md=dict(dialnorm=3, bsmod=2), **c["kw"]), got)
    finally:
        _restore(engine)


def test_per_frame_words_with_state_slots_and_tiles(engine):
    """the array goes by the frame's position in the call: state slots do not move it, a tile reads its own slice"""
    import torch
    S, F = 10, 2
    pcm = T.content("music", 6, S, F, seed=41)
    words = _random_words(np.random.default_rng(8), S, F)
    try:
        plain = T.encode(engine, pcm)
        engine.set_encode_metadata_frames(_words_tensor(words))
        want = T.encode(engine, pcm)
        _check_frames_carry_words(want, plain, words, 7)
        perm = torch.from_numpy(np.random.default_rng(3).permutation(S).astype(np.int32)).cuda()
        engine._check(engine.lib.ac3mi_set_state_slots(ctypes.c_void_p(engine.ctx), ctypes.c_void_p(perm.data_ptr())))
        assert np.array_equal(T.encode(engine, pcm), want), "slots"
        engine.set_tile_frames(3 * F)
        assert np.array_equal(T.encode(engine, pcm), want), "slots + tiles"
        engine._check(engine.lib.ac3mi_set_state_slots(ctypes.c_void_p(engine.ctx), None))
        assert np.array_equal(T.encode(engine, pcm), want), "tiles"
    finally:
        _restore(engine)


@pytest.mark.parametrize("nch,pack,layout", [(2, 2, None), (6, 1, None), (2, 1, (1, 0, 0))])
def test_per_frame_words_under_drc(engine, nch, pack, layout):
    """every stream its own dialnorm (one of them the reserved 0, coded as 31): stream s's bytes and DRC state are those of
    encoding it alone under ac3mi_set_encode_metadata with that dialnorm"""
    import torch
    S, F = 8, 3
    kw = dict(layout=layout) if layout else {}
    kinds = ("music", "tones", "noise", "quiet", "bursts")
    pcm = np.stack([H.gen_pcm(F, nch, seed=500 + s, kind=kinds[s % 5]) for s in range(S)])
    dn = [0, 1, 9, 17, 24, 27, 30, 31]
    rest = dict(bsmod=3, cmixlev=2, surmixlev=0, dsurmod=1, copyrightb=1, origbs=0)
    words = np.array([[M.pack_word(dialnorm=d, **rest)] * F for d in dn])
    try:
        state = torch.tensor([0, 40, -300, 7, 0, 100, -50, 0], dtype=torch.int32, device="cuda")
        state0 = state.clone()
        engine.set_encode_metadata_frames(_words_tensor(words))
        got = T.encode(engine, pcm, pack=pack, drc=1, state=state, **kw)
        engine.set_encode_metadata_frames(None)
        got_state = state.cpu().numpy()
        for s in range(S):
            st = state0[s:s + 1].clone()
            alone = T.encode(engine, pcm[s:s + 1], pack=pack, drc=1, state=st, md=dict(dialnorm=dn[s] or 31, **rest), **kw)
            assert np.array_equal(got[s], alone[0]), s
            assert int(st.cpu()[0]) == int(got_state[s]), s
        # the dialnorm matters: stream 1 (dialnorm 1) coded at dialnorm 31 differs
        st = state0[1:2].clone()
        other = T.encode(engine, pcm[1:2], pack=pack, drc=1, state=st, md=dict(dialnorm=31, **rest), **kw)
        assert not np.array_equal(other[0], got[1])
    finally:
        _restore(engine)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the transcode that follows its source

CTX = dict(dialnorm=20, bsmod=3, cmixlev=2, surmixlev=0, dsurmod=1, copyrightb=1, origbs=0)


def _transcode(engine, batch, fb, acmod, lfeon, flags, rate, chmap, s_base=0):
    """batch [S][F][stride] -> dict of host arrays (frames, status and the four state arrays); stream s starts its dither
    generator at 5 (s_base + s) + 1"""
    import torch
    pkg = H.pkg()
    S, F, _ = batch.shape
    dec = pkg.DecodeDesc(flags=flags, level=1.0, bias=384.0, dynrng=1, acmod=acmod, lfeon=lfeon, frame_bytes=fb)
    n_out, _ = engine.decode_planes(dec)
    enc = pkg.EncodeDesc(48000, rate, n_out)
    delay = torch.zeros((S, n_out, 128), dtype=torch.float32, device="cuda")
    lfsr = ((torch.arange(S, dtype=torch.int32) + s_base) * 5 + 1).to(torch.int16).cuda()
    last = torch.zeros((S, n_out, 256), dtype=torch.int16, device="cuda")
    csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
    out, status = engine.transcode_batch(dec, enc, torch.from_numpy(np.ascontiguousarray(batch)).cuda(), delay, lfsr, chmap, last, csnr)
    engine.sync()
    return dict(frames=out.cpu().numpy()[:, :, :enc.frame_bytes()], status=status.cpu().numpy().astype(np.uint32),
                delay=delay.cpu().numpy(), lfsr=lfsr.cpu().numpy(), last=last.cpu().numpy(), csnr=csnr.cpu().numpy())


def _patch(frame, **fields):
    """overwrites fixed-width BSI fields of a frame in place"""
    P = M.parse_head(frame)
    bits = np.unpackbits(frame)
    for k, v in fields.items():
        n = M.WIDTH[k]
        bits[P.pos[k]:P.pos[k] + n] = [(v >> (n - 1 - i)) & 1 for i in range(n)]
    frame[:] = np.packbits(bits)


def _follow_case(engine, groups, acmod, lfeon, flags, rate, chmap, coded_acmod, layout=0, tile=0):
    """groups: list of [streams][F][fb] source arrays, every frame of a group carrying the same metadata.  One mode-1 call over
    all of them against one mode-0 call per group under the model's word; the last frame of the last stream has its sync word
    zeroed."""
    fb = groups[0].shape[2]
    F = groups[0].shape[1]
    stride = (fb + 3) & ~3
    src = np.concatenate(groups)
    S = src.shape[0]
    batch = np.zeros((S, F, stride), np.uint8)
    batch[:, :, :fb] = src
    rs, rf = S - 1, F - 1 if F > 1 else 0                             # the refused frame: last stream, last frame
    batch[rs, rf, :2] = 0
    ctx_word = M.pack_word(**CTX)
    want_words = np.zeros((S, F), np.int64)
    for s in range(S):
        for f in range(F):
            refused = (s, f) == (rs, rf)
            want_words[s, f] = M.followed_word(None if refused else M.parse_head(batch[s, f]), coded_acmod, ctx_word, refused)
    try:
        engine.set_encode_layout(layout)
        engine.set_encode_metadata(**CTX)
        engine.set_encode_metadata_source(1)
        engine.set_tile_frames(tile)
        # an array of ac3mi_set_encode_metadata_frames is ignored by such a transcode
        engine.set_encode_metadata_frames(_words_tensor(np.full((S, F), M.pack_word(dialnorm=5, bsmod=6))))
        got = _transcode(engine, batch, fb, acmod, lfeon, flags, rate, chmap)
        engine.set_encode_metadata_frames(None)
        engine.set_encode_metadata_source(0)
        engine.set_tile_frames(131072)
        assert got["status"][rs, rf] & 0x1ff == 0x100 | 0x3f and (np.delete(got["status"].ravel(), rs * F + rf) & 0x1ff == 0).all()
        assert _crc_ok(engine, got["frames"])
        s0 = 0
        for g in groups:
            n = g.shape[0]
            sl = slice(s0, s0 + n)
            word = int(want_words[s0, 0])
            engine.set_encode_metadata(**M.fields_of(word))
            ref = _transcode(engine, batch[sl], fb, acmod, lfeon, flags, rate, chmap, s_base=s0)
            for k in ("status", "delay", "lfsr", "last", "csnr"):
                assert np.array_equal(got[k][sl], ref[k]), (k, s0)
            for s in range(n):
                for f in range(F):
                    a, b = got["frames"][s0 + s, f], ref["frames"][s, f]
                    P = A.parse_frame(a)
                    assert P.acmod == coded_acmod
                    want = M.coded_fields(int(want_words[s0 + s, f]), coded_acmod)
                    assert {k: P.fields[k] for k in want} == want, (s0 + s, f)
                    if (s0 + s, f) == (rs, rf):
                        # the refused frame: the context's word on the same silence - equal outside the metadata and the CRC words
                        assert int(want_words[rs, rf]) == ctx_word and word != ctx_word
                        x, y = np.unpackbits(a), np.unpackbits(b)
                        free = np.zeros(x.size, bool)
                        free[M.metadata_bits(P)] = True
                        free[16:32] = True
                        free[-16:] = True
                        assert np.array_equal(x[~free], y[~free]) and not np.array_equal(a, b)
                    else:
                        assert int(want_words[s0 + s, f]) == word, "a group shares one word"
                        assert np.array_equal(a, b), (s0 + s, f)
            s0 += n
        return got, want_words
    finally:
        _restore(engine)


def _groups_51(engine, F):
    """three groups of 5.1 sources coded under three metadata settings + packer streams holding reserved codes"""
    mds = (dict(dialnorm=24, cmixlev=0, surmixlev=2, copyrightb=1, origbs=0, bsmod=1),
           dict(dialnorm=31, cmixlev=1, surmixlev=1),
           dict(dialnorm=11, cmixlev=2, surmixlev=0, bsmod=4, origbs=1))
    groups = [T.encode(engine, T.tones(7, 1, 3, F, seed=700 + i), md=md) for i, md in enumerate(mds)]
    pk = np.stack([packer.make_stream(7100 + s, F, 7, 1, frmsizecod=28, features=dict(bsi_opts=(0.0, 1.0)[s])) for s in range(2)])
    for fr in pk.reshape(-1, pk.shape[2]):
        _patch(fr, dialnorm=0, bsmod=6, cmixlev=3, surmixlev=3, copyrightb=0, origbs=0)
    groups.insert(1, pk)
    assert all(g.shape[2] == 1536 for g in groups)
    return groups


@pytest.mark.parametrize("tile", [0, 1])
def test_transcode_follows_source_51(engine, tile):
    """5.1 to 5.1, untiled and in tiles smaller than the batch: dialnorm, bsmod, copyrightb, origbs, cmixlev and surmixlev are the
    source's (sanitised), byte for byte the mode-0 transcode of each group under that word"""
    F = 3
    groups = _groups_51(engine, F)
    got, words = _follow_case(engine, groups, 7, 1, 7 | 16, 448000, H.CHMAP6, 7, tile=4 * F if tile else 0)
    f = M.fields_of(int(words[0, 0]))
    assert (f["dialnorm"], f["cmixlev"], f["surmixlev"], f["copyrightb"], f["origbs"], f["dsurmod"]) == (24, 0, 2, 1, 0, 1)
    f = M.fields_of(int(words[3, 0]))                                   # the packer group: reserved codes sanitised
    assert (f["dialnorm"], f["bsmod"], f["cmixlev"], f["surmixlev"]) == (31, 6, 1, 1)


def test_transcode_follows_source_through_a_downmix(engine):
    """5.1 to STEREO: the coded 2/0 sends dsurmod, which no 3/2 source carries - the context's; dialnorm and the rest carry"""
    F = 2
    groups = _groups_51(engine, F)
    got, words = _follow_case(engine, groups, 7, 1, 2, 192000, (0, 1), 2)
    f = M.fields_of(int(words[0, 0]))
    assert (f["dialnorm"], f["bsmod"], f["copyrightb"], f["origbs"], f["dsurmod"]) == (24, 1, 1, 0, CTX["dsurmod"])
    assert (f["cmixlev"], f["surmixlev"]) == (CTX["cmixlev"], CTX["surmixlev"])


def test_transcode_follows_source_layout_mode_2(engine):
    """a 2/0+LFE source under ac3mi_set_encode_layout 2 stays 2/0+LFE and keeps its dsurmod"""
    F = 2
    mds = (dict(dialnorm=27, dsurmod=2, bsmod=2), dict(dialnorm=14, dsurmod=0, copyrightb=1), dict(dialnorm=31, dsurmod=1, origbs=0))
    groups = [T.encode(engine, T.tones(2, 1, 3, F, seed=800 + i), layout=(1, 2, 1), md=md) for i, md in enumerate(mds)]
    got, words = _follow_case(engine, groups, 2, 1, 2 | 16, 384000, None, 2, layout=2)
    assert [M.fields_of(int(words[3 * i, 0]))["dsurmod"] for i in range(3)] == [2, 0, 1]
    assert all(A.parse_frame(f).lfeon == 1 for f in got["frames"].reshape(-1, got["frames"].shape[2]))


def test_refusals_take_the_context_word(engine):
    """what the decoder refuses, the follower does not read: a frame of another acmod, and a frame ac3mi_set_decode_crc 2
    conceals"""
    F = 2
    src = T.encode(engine, T.tones(7, 1, 8, F, seed=900), md=dict(dialnorm=9, cmixlev=0, surmixlev=2, bsmod=5))
    batch = src.copy()
    batch[2, 1, 1000] ^= 0x10                                          # damaged mantissas: CRC2 fails
    other = T.encode(engine, T.tones(2, 0, 1, 1, seed=901), rate=384000, md=dict(dialnorm=4))[0, 0]
    assert other.shape[0] == 1536
    batch[5, 0] = other                                                # a 2/0 frame in a 3/2+LFE batch
    try:
        engine.set_encode_metadata(**CTX)
        engine.set_encode_metadata_source(1)
        engine.set_decode_crc(2)
        got = _transcode(engine, batch, 1536, 7, 1, 7 | 16, 448000, H.CHMAP6)
        want_src = M.coded_fields(M.followed_word(M.parse_head(src[0, 0]), 7, M.pack_word(**CTX)), 7)
        want_ctx = M.coded_fields(M.pack_word(**CTX), 7)
        assert want_src["dialnorm"] == 9 and want_ctx["dialnorm"] == 20
        for s in range(8):
            for f in range(F):
                refused = (s, f) in ((2, 1), (5, 0))
                assert bool(got["status"][s, f] & 0x100) == refused, (s, f)
                P = A.parse_frame(got["frames"][s, f])
                want = want_ctx if refused else want_src
                assert {k: P.fields[k] for k in want} == want, (s, f)
        assert got["status"][2, 1] & 0x800
    finally:
        _restore(engine)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the defaults

def test_defaults_and_bad_modes(engine):
    import torch
    pkg = H.pkg()
    lib, ctx = engine.lib, ctypes.c_void_p(engine.ctx)
    S, F = 8, 2
    pcm = T.content("music", 6, S, F, seed=61)
    fresh = pkg.Engine(0)
    try:
        want_enc = T.encode(fresh, pcm)
        src = np.zeros((S, F, 1536), np.uint8)
        src[:] = want_enc
        want_tc = _transcode(fresh, src, 1536, 7, 1, 7 | 16, 448000, H.CHMAP6)
        ws_fresh = fresh.workspace_bytes()
    finally:
        fresh.close()
    try:
        engine.set_encode_metadata_frames(_words_tensor(_random_words(np.random.default_rng(1), S, F)))
        engine.set_encode_metadata_source(1)
        assert not np.array_equal(T.encode(engine, pcm), want_enc)
        assert lib.ac3mi_set_encode_metadata_source(ctx, 2) == ERR_ARG and lib.ac3mi_set_encode_metadata_source(ctx, -1) == ERR_ARG
        assert lib.ac3mi_set_encode_metadata_source(None, 0) == ERR_ARG and lib.ac3mi_set_encode_metadata_frames(None, None) == ERR_ARG
        before = engine.workspace_bytes()
        changed = _transcode(engine, src, 1536, 7, 1, 7 | 16, 448000, H.CHMAP6)      # still mode 1: the bad modes left it
        assert np.array_equal(changed["frames"], want_tc["frames"])                  # (the source carries the defaults)
        engine.set_encode_metadata(dialnorm=12)
        still = _transcode(engine, src, 1536, 7, 1, 7 | 16, 448000, H.CHMAP6)
        assert np.array_equal(still["frames"], want_tc["frames"]), "mode 1 survived the bad modes: the source's dialnorm, not 12"
        assert engine.workspace_bytes() >= before and engine.workspace_bytes() >= 4 * S * F
        engine.set_encode_metadata()
        engine.set_encode_metadata_frames(None)
        engine.set_encode_metadata_source(0)
        assert np.array_equal(T.encode(engine, pcm), want_enc)
        back = _transcode(engine, src, 1536, 7, 1, 7 | 16, 448000, H.CHMAP6)
        for k in want_tc:
            assert np.array_equal(back[k], want_tc[k]), k
    finally:
        _restore(engine)
