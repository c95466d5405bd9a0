"""GPU: dynrng and compr words from the caller (ac3mi_set_encode_dynrng_frames) and from a transcode's source
(ac3mi_set_encode_drc_source 1), against tests/dynrng_model.py, the frame reader (tests/ac3_syntax.py), the bit-budget audit
of test_frame_budget_gpu.py and the decoder's own dynamic-range tap.  Batches of 2 to 77 frames."""
import ctypes

import numpy as np
import pytest

from tests import _harness as H
from tests import _tools as T
from tests import ac3_syntax as A
from tests import dynrng_model as D
from tests import packer
from tests import test_frame_budget_gpu as B

pytestmark = pytest.mark.gpu

ERR_ARG = -1
FEATURES = dict(dynrng=0.5, bsi_opts=0.5, dsur=0.0)


def _restore(engine):
    engine.set_encode_dynrng_frames(None, None)
    engine.set_encode_drc_source(0)
    engine.set_encode_drc(0)
    engine.set_encode_layout(0)
    engine.set_encode_mode(0)
    engine.set_decode_mode(0)
    engine.set_decode_crc(0)
    engine.set_fixed_shape(1)
    engine.set_tile_frames(131072)


def _tensors(codes, compr):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(codes, np.uint8)).cuda() if codes is not None else None
    c = torch.from_numpy(np.ascontiguousarray(compr).astype(np.uint16).view(np.int16)).cuda() if compr is not None else None
    return d, c


def _random_arrays(rng, S, F, density=0.5):
    """codes [S][F][6][2]: a new random word in a block with probability `density` (0 among them), else the block before's
    (block 0: 0); compr [S][F][2]: half of them sent, junk in bits 9-15"""
    codes = np.zeros((S, F, 6, 2), np.uint8)
    new = rng.random((S, F, 6, 2)) < density
    word = rng.integers(0, 256, (S, F, 6, 2))
    word[rng.random((S, F, 6, 2)) < 0.1] = 0
    for b in range(6):
        prev = codes[:, :, b - 1] if b else np.zeros((S, F, 2), np.uint8)
        codes[:, :, b] = np.where(new[:, :, b], word[:, :, b], prev)
    compr = rng.integers(0, 256, (S, F, 2)) | (rng.integers(0, 2, (S, F, 2)) << 8) | (rng.integers(0, 128, (S, F, 2)) << 9)
    return codes, compr.astype(np.uint16)


def _transcode(engine, batch, fb, acmod, lfeon, flags, rate, chmap, dynrng=0):
    """batch [S][F][stride] -> dict of host arrays: frames, status and the four state arrays (T.transcode decodes with dynrng 1
    and asserts a clean status: this feature needs neither)"""
    import torch
    pkg = H.pkg()
    S, F, _ = batch.shape
    dec = pkg.DecodeDesc(flags=flags, level=1.0, bias=384.0, dynrng=dynrng, acmod=acmod, lfeon=lfeon, frame_bytes=fb)
    n_out, _ = engine.decode_planes(dec)
    enc = pkg.EncodeDesc(48000, rate, n_out)
    delay = torch.zeros((S, n_out, 128), dtype=torch.float32, device="cuda")
    lfsr = (torch.arange(S, dtype=torch.int32) * 5 + 1).to(torch.int16).cuda()
    last = torch.zeros((S, n_out, 256), dtype=torch.int16, device="cuda")
    csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
    out, status = engine.transcode_batch(dec, enc, torch.from_numpy(np.ascontiguousarray(batch)).cuda(), delay, lfsr, chmap, last, csnr)
    engine.sync()
    return dict(frames=out.cpu().numpy()[:, :, :enc.frame_bytes()], status=status.cpu().numpy().astype(np.uint32),
                delay=delay.cpu().numpy(), lfsr=lfsr.cpu().numpy(), last=last.cpu().numpy(), csnr=csnr.cpu().numpy())


def _padded(src):
    S, F, fb = src.shape
    batch = np.zeros((S, F, (fb + 3) & ~3), np.uint8)
    batch[:, :, :fb] = src
    return batch


def _crc_ok(engine, frames):
    import torch
    fb = frames.shape[-1]
    v = engine.crc_check_batch(torch.from_numpy(_padded(frames.reshape(1, -1, fb))[0]).cuda(), fb)
    engine.sync()
    return not v.cpu().numpy().any()


_POOL = {}


def _source(acmod, lfeon, frmsizecod, S, F, seed):
    """[S][F][fb] packer frames carrying dynrng and compr words (a stream is any sequence of them: every frame sends all it
    needs in block 0); the frames of a layout are made once and dealt out"""
    key = (acmod, lfeon, frmsizecod)
    need = 24
    while True:
        try:
            if key not in _POOL or len(_POOL[key]) < need:
                _POOL[key] = packer.make_stream(6000 + 16 * acmod + lfeon, need, acmod, lfeon, frmsizecod=frmsizecod, features=FEATURES)
            break
        except RuntimeError:            # the packer cannot fit a frame: a larger one
            frmsizecod += 2
    pool = _POOL[key]
    pick = np.random.default_rng(seed).integers(0, len(pool), S * F)
    pick[:len(pool)] = np.arange(len(pool))[:S * F]
    return pool[pick].reshape(S, F, -1)


# ---------------------------------------------------------------------------------------------------------------------
# 1. off means unchanged

def test_off_means_unchanged(engine):
    import torch
    pkg = H.pkg()
    S, F = 3, 2
    pcms = {nch: T.content("music", nch, S, F, seed=20 + nch) for nch in (1, 2, 6)}
    fresh = pkg.Engine(0)
    try:
        want = {nch: T.encode(fresh, p) for nch, p in pcms.items()}
        want_tc = _transcode(fresh, _padded(want[6]), 1536, 7, 1, 7 | 16, 448000, H.CHMAP6)
    finally:
        fresh.close()
    try:
        for zero in (False, True):
            if zero:
                engine.set_encode_dynrng_frames(torch.zeros((S, F, 6, 2), dtype=torch.uint8, device="cuda"),
                                                torch.zeros((S, F, 2), dtype=torch.int16, device="cuda"))
            for nch, p in pcms.items():
                assert np.array_equal(T.encode(engine, p), want[nch]), (zero, nch)
            got = _transcode(engine, _padded(want[6]), 1536, 7, 1, 7 | 16, 448000, H.CHMAP6)
            for k in want_tc:
                assert np.array_equal(got[k], want_tc[k]), (zero, k)
    finally:
        _restore(engine)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the arrays reach the frames

CONFIGS = {"1/0": dict(nch=1, acmod=1, lfeon=0, kw={}),
           "2/0": dict(nch=2, acmod=2, lfeon=0, kw={}),
           "3/2+LFE": dict(nch=6, acmod=7, lfeon=1, kw={}),
           "dual mono": dict(nch=2, acmod=0, lfeon=0, kw=dict(layout=(1, 0, 0))),
           "2/0 coupled": dict(nch=2, acmod=2, lfeon=0, kw=dict(cpl=(1, 2)))}


@pytest.mark.parametrize("pack", [1, 2])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_arrays_reach_the_frames(engine, config, pack):
    """every dynrnge / dynrng / dynrng2e / dynrng2 and compr field is sends() of the arrays; CRCs, clean decode, and the bit
    budget: a search that misses a word's 8 bits fails the audit's accounting, one that over-counts its search item"""
    c = CONFIGS[config]
    S, F = 5, 3
    pcm = T.content("music", c["nch"], S, F, seed=100 + c["nch"])
    codes, compr = _random_arrays(np.random.default_rng(31 + pack), S, F)
    assert not np.array_equal(codes[..., 0], codes[..., 1])
    rate = B.RATES[c["nch"]][1]
    try:
        engine.set_encode_dynrng_frames(*_tensors(codes, compr))
        frames, taps = T.encode(engine, pcm, pack=pack, rate=rate, taps=True, **c["kw"])
        nd, nc = D.check_frames(frames, codes, compr, c["acmod"])
        assert nd > 10 and nc > 2
        if "cpl" in c["kw"]:
            assert any(T.coupling_view(f, c["nch"])[0] for f in frames.reshape(-1, frames.shape[2])), "no frame coupled"
        rep = B.Report()
        B.audit(rep, frames, taps, np.full(S, 40), "%s pack %d" % (config, pack))
        rep.finish("arrays %s" % config)
        assert rep.n["dynrng"] + rep.n["dynrng2"] == nd
        engine.set_encode_dynrng_frames(None, None)
        T.decodes_cleanly(frames, c["acmod"], c["lfeon"], engine)
    finally:
        _restore(engine)


def test_compr_with_a_profile(engine):
    """d_compr beside ac3mi_set_encode_drc: the profile's dynrng words (block 0 always sends; dual mono the same word twice) and
    bytes outside the compr fields' cost stay; the array's compr words are coded and budgeted"""
    import torch
    S, F = 3, 2
    pcm = T.content("music", 2, S, F, seed=77)
    _, compr = _random_arrays(np.random.default_rng(9), S, F)
    compr[0, 0] |= 0x100
    try:
        for kw, acmod in ((dict(layout=(1, 0, 0)), 0), ({}, 2)):
            plain = T.encode(engine, pcm, drc=1, rate=256000, **kw)
            engine.set_encode_dynrng_frames(None, _tensors(None, compr)[1])
            frames, taps = T.encode(engine, pcm, drc=1, rate=256000, taps=True, **kw)
            engine.set_encode_dynrng_frames(None, None)
            rep = B.Report()
            B.audit(rep, frames, taps, np.full(S, 40), "profile + compr acmod %d" % acmod)
            rep.finish("profile + compr")
            for s in range(S):
                for f in range(F):
                    P, Q = A.parse_frame(frames[s, f]), A.parse_frame(plain[s, f])
                    for p, sfx in enumerate(("", "2") if acmod == 0 else ("",)):
                        want = int(compr[s, f, p])
                        assert P.fields["compr%se" % sfx] == (want >> 8) & 1 and P.fields.get("compr" + sfx, 0) == ((want & 0xff) if want & 0x100 else 0)
                    for b in range(6):
                        for k in ("dynrnge", "dynrng", "dynrng2e", "dynrng2"):
                            assert P.blocks[b].fields.get(k) == Q.blocks[b].fields.get(k), (s, f, b, k)
                    assert P.blocks[0].fields["dynrnge"] == 1
    finally:
        _restore(engine)


# ---------------------------------------------------------------------------------------------------------------------
# 3. one call equals split calls; tiles read their own slices

def test_one_call_equals_split_calls(engine):
    import torch
    S, F = 4, 3
    pcm = T.content("music", 2, S, F, seed=55)
    codes, compr = _random_arrays(np.random.default_rng(2), S, F)
    kw = dict(layout=(1, 0, 0), rate=256000)
    try:
        engine.set_encode_dynrng_frames(*_tensors(codes, compr))
        want = T.encode(engine, pcm, **kw)
        D.check_frames(want, codes, compr, 0)
        last = torch.zeros((S, 2, 256), dtype=torch.int16, device="cuda")
        csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
        engine.set_encode_dynrng_frames(*_tensors(codes[:, :1], compr[:, :1]))
        a = T.encode(engine, pcm[:, :1536], last=last, csnr=csnr, **kw)
        engine.set_encode_dynrng_frames(*_tensors(codes[:, 1:], compr[:, 1:]))
        b = T.encode(engine, pcm[:, 1536:], last=last, csnr=csnr, **kw)
        assert np.array_equal(np.concatenate([a, b], 1), want)
    finally:
        _restore(engine)


def test_tiles_read_their_slices(engine):
    S, F = 6, 2
    pcm = T.content("music", 6, S, F, seed=56)
    codes, compr = _random_arrays(np.random.default_rng(3), S, F)
    try:
        engine.set_encode_dynrng_frames(*_tensors(codes, compr))
        want = T.encode(engine, pcm, rate=448000)
        D.check_frames(want, codes, compr, 7)
        engine.set_tile_frames(4)
        assert np.array_equal(T.encode(engine, pcm, rate=448000), want)
        engine.set_tile_frames(131072)
        src = _padded(want)
        a = _transcode(engine, src, want.shape[2], 7, 1, 7 | 16, 448000, H.CHMAP6)
        D.check_frames(a["frames"], codes, compr, 7)
        engine.set_tile_frames(4)
        b = _transcode(engine, src, want.shape[2], 7, 1, 7 | 16, 448000, H.CHMAP6)
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    finally:
        _restore(engine)


# ---------------------------------------------------------------------------------------------------------------------
# 4. source mode equals the model

#        name: source acmod, lfeon, frmsizecod | request flags, rate, chmap, layout mode | coded acmod, programme | S, F, fixed
SOURCE_CASES = {
    "5.1 11x7": (7, 1, 30, 7 | 16, 448000, H.CHMAP6, 0, 7, -1, 11, 7, None),
    "5.1 70x1 fixed shape": (7, 1, 30, 7 | 16, 448000, H.CHMAP6, 0, 7, -1, 70, 1, 1),
    "2/0": (2, 0, 20, 2, 192000, (0, 1), 0, 2, -1, 5, 3, None),
    "1/0": (1, 0, 16, 1, 192000, (0,), 0, 1, -1, 5, 3, None),
    "5.1 to stereo": (7, 1, 30, 2, 192000, (0, 1), 0, 2, -1, 5, 3, None),
    "dual mono kept": (0, 0, 20, 0, 192000, None, 2, 0, -1, 5, 3, None),
    "dual mono CHANNEL2": (0, 0, 20, 9, 192000, (0,), 0, 1, 1, 5, 3, None),
}


def _source_case(engine, name, status_of=None, damage=None, crc=0, modes=(1, 3, 4, 5, 6)):
    """mode 1 under every decode mode: the words of the output are sends(effective(source)), the bytes and the state those of a
    mode-0 transcode given the model's arrays.  damage(batch): damages source frames in place; status_of(status) checks the
    status words.  Returns (source batch, its frame size, model codes, model compr, one output)"""
    acmod, lfeon, fsc, flags, rate, chmap, layout, coded, prog, S, F, fixed = SOURCE_CASES[name]
    src = _source(acmod, lfeon, fsc, S, F, seed=len(name))
    fb = src.shape[2]
    batch = _padded(src)
    if damage:
        damage(batch)
    parsed = {}
    out = None
    try:
        engine.set_encode_layout(layout)
        engine.set_decode_crc(crc)
        if fixed is not None:
            engine.set_fixed_shape(fixed)
        for mode in modes:
            engine.set_decode_mode(mode)
            engine.set_encode_drc_source(1)
            # arrays of ac3mi_set_encode_dynrng_frames are ignored by such a transcode
            engine.set_encode_dynrng_frames(*_tensors(np.full((S, F, 6, 2), 0x55, np.uint8), np.full((S, F, 2), 0x1aa, np.uint16)))
            got = _transcode(engine, batch, fb, acmod, lfeon, flags, rate, chmap)
            engine.set_encode_drc_source(0)
            engine.set_encode_dynrng_frames(None, None)
            plain = _transcode(engine, batch, fb, acmod, lfeon, flags, rate, chmap)
            assert np.array_equal(got["status"], plain["status"]), (mode, "the status words are mode 0's")
            if status_of:
                status_of(got["status"])
            else:
                assert (got["status"] & 0x1ff).max() == 0
            if out is None:
                codes, compr = D.effective(batch[:, :, :fb], got["status"], prog)
                assert D.sends(codes).sum() > S * F and (compr & 0x100).any(), "the sources carry words"
            key = got["frames"].tobytes()
            if key not in parsed:
                D.check_frames(got["frames"], codes, compr, coded)
                assert _crc_ok(engine, got["frames"])
                parsed[key] = mode
            engine.set_encode_dynrng_frames(*_tensors(codes, compr))
            ref = _transcode(engine, batch, fb, acmod, lfeon, flags, rate, chmap)
            engine.set_encode_dynrng_frames(None, None)
            for k in ref:
                assert np.array_equal(got[k], ref[k]), (mode, k)
            assert not np.array_equal(got["frames"], plain["frames"])
            out = got
        return batch, fb, codes, compr, out
    finally:
        _restore(engine)


@pytest.mark.parametrize("name", list(SOURCE_CASES))
def test_source_mode_equals_the_model(engine, name):
    _source_case(engine, name)


def test_source_without_words_gives_mode_0(engine):
    S, F = 4, 2
    src = _padded(T.encode(engine, T.content("music", 6, S, F, seed=13)))
    try:
        want = _transcode(engine, src, 1536, 7, 1, 7 | 16, 448000, H.CHMAP6)
        engine.set_encode_drc_source(1)
        for mode in (0, 1, 5):
            engine.set_decode_mode(mode)
            got = _transcode(engine, src, 1536, 7, 1, 7 | 16, 448000, H.CHMAP6)
            for k in want:
                assert np.array_equal(got[k], want[k]), (mode, k)
    finally:
        _restore(engine)


# ---------------------------------------------------------------------------------------------------------------------
# 5. an independent check through the decoder

def _gains(engine, frames, acmod, lfeon):
    """the gain in force in every block and programme, [S][F][6][2], from the decoder's dynamic-range tap (dynrng 1)"""
    _, status, taps = T.decode(engine, np.ascontiguousarray(frames), acmod, lfeon, taps=True)
    assert (status & 0x1ff).max() == 0
    g = taps["dynrng"].copy()
    prev = np.ones(g[:, :, 0].shape, np.float32)
    for b in range(6):
        g[:, :, b] = np.where(np.isnan(g[:, :, b]), prev, g[:, :, b])
        prev = g[:, :, b]
    return g


@pytest.mark.parametrize("name", ["5.1 11x7", "dual mono kept"])
def test_decoder_sees_the_same_gains(engine, name):
    acmod, lfeon = SOURCE_CASES[name][:2]
    batch, fb, codes, compr, out = _source_case(engine, name, modes=(0,))
    a = _gains(engine, batch[:, :, :fb], acmod, lfeon)
    b = _gains(engine, out["frames"], acmod, lfeon)
    nprog = 2 if acmod == 0 else 1
    assert np.array_equal(a[..., :nprog].view(np.uint32), b[..., :nprog].view(np.uint32))
    assert len(np.unique(a[..., :nprog])) > 8
    want = np.vectorize(D.gain)(codes[..., :nprog]).astype(np.float32)
    assert np.array_equal(a[..., :nprog], want)


# ---------------------------------------------------------------------------------------------------------------------
# 6. damaged frames carry nothing

def test_refused_frames_carry_nothing(engine):
    """bytes 0-1 of one frame per stream zeroed: status 0x13f, no words in the new frame; the neighbours carry theirs (the
    model resolves from the status words, which are mode 0's)"""
    S, F = 5, 3

    def damage(batch):
        for s in range(S):
            batch[s, s % F, :2] = 0

    def status_of(status):
        for s in range(S):
            for f in range(F):
                assert (status[s, f] & 0x1ff) == (0x13f if f == s % F else 0), (s, f)

    _, _, codes, compr, out = _source_case(engine, "2/0", status_of, damage, modes=(1, 3, 4))
    for s in range(S):
        assert not codes[s, s % F].any() and not compr[s, s % F].any()
        P = A.parse_frame(out["frames"][s, s % F])
        assert not P.fields["compre"] and not any(Bk.fields["dynrnge"] for Bk in P.blocks)
    assert D.sends(codes).sum() > S


def test_concealed_frames_carry_nothing(engine):
    """ac3mi_set_decode_crc 2 and one flipped mantissa bit: the concealed frame carries no words"""
    S, F = 4, 3
    pcm = T.content("music", 6, S, F, seed=91)
    codes, compr = _random_arrays(np.random.default_rng(17), S, F)
    try:
        engine.set_encode_dynrng_frames(*_tensors(codes, compr))
        src = _padded(T.encode(engine, pcm, rate=448000))
        engine.set_encode_dynrng_frames(None, None)
        fb = src.shape[2]
        hit = [(s, (s + 1) % F) for s in range(S)]
        for s, f in hit:
            src[s, f, fb - 40] ^= 0x08
        for mode in (3, 4):
            engine.set_decode_mode(mode)
            engine.set_decode_crc(2)
            plain = _transcode(engine, src, fb, 7, 1, 7 | 16, 448000, H.CHMAP6)
            engine.set_encode_drc_source(1)
            got = _transcode(engine, src, fb, 7, 1, 7 | 16, 448000, H.CHMAP6)
            engine.set_encode_drc_source(0)
            assert np.array_equal(got["status"], plain["status"])
            want_c, want_k = codes.copy(), compr.copy()
            for s in range(S):
                for f in range(F):
                    assert bool(got["status"][s, f] & 0x100) == ((s, f) in hit) and bool(got["status"][s, f] & 0x800) == ((s, f) in hit)
                    if (s, f) in hit:
                        want_c[s, f] = 0
                        want_k[s, f] = 0
            D.check_frames(got["frames"], want_c, want_k, 7)
    finally:
        _restore(engine)


def test_frames_with_a_failed_block_carry_nothing(engine):
    """a chbwcod above 60 (A/52 5.4.3.24; liba52 returns 1, parse.c:673-678) in block 0, 2 or 5 of three frames: the block's
    status bit and those after it, not bit 8 - and no words, though the blocks before the error were read"""
    S, F = 5, 3
    where = {(0, 1): 0, (2, 0): 2, (3, 2): 5}

    def damage(batch):
        for (s, f), blk in where.items():
            P = A.parse_frame(batch[s, f])
            names = [k for k in P.blocks[blk].pos if k.startswith("chbwcod")]
            while not names:            # (the block reuses every channel's exponents: an earlier one)
                blk -= 1
                names = [k for k in P.blocks[blk].pos if k.startswith("chbwcod")]
            where[(s, f)] = blk
            p = P.blocks[blk].pos[names[0]]
            bits = np.unpackbits(batch[s, f])
            bits[p:p + 6] = 1
            batch[s, f] = np.packbits(bits)
            assert H.orc_decode(batch[s, f:f + 1, :P.frame_bytes], 2, 1.0, 0.0)[1] > 0

    def status_of(status):
        for s in range(S):
            for f in range(F):
                blk = where.get((s, f))
                want = 0 if blk is None else (0x3f << blk) & 0x3f
                assert (status[s, f] & 0x1ff) == want, (s, f, hex(status[s, f]))

    _, _, codes, compr, out = _source_case(engine, "2/0", status_of, damage, modes=(1, 3, 4, 5))
    for s, f in where:
        assert not codes[s, f].any() and not compr[s, f].any()
        P = A.parse_frame(out["frames"][s, f])
        assert not P.fields["compre"] and not any(Bk.fields["dynrnge"] for Bk in P.blocks)


# ---------------------------------------------------------------------------------------------------------------------
# 7. validation

def test_validation(engine):
    import torch
    lib, ctx = engine.lib, ctypes.c_void_p(engine.ctx)
    S, F = 3, 2
    pcm = T.content("music", 6, S, F, seed=5)
    codes, compr = _random_arrays(np.random.default_rng(4), S, F)
    d, c = _tensors(codes, compr)
    state = torch.zeros((S,), dtype=torch.int32, device="cuda")
    try:
        src = _padded(T.encode(engine, pcm))
        # mode outside 0..1; a null context
        assert lib.ac3mi_set_encode_drc_source(ctx, 2) == ERR_ARG and lib.ac3mi_set_encode_drc_source(ctx, -1) == ERR_ARG
        assert lib.ac3mi_set_encode_drc_source(None, 0) == ERR_ARG and lib.ac3mi_set_encode_dynrng_frames(None, None, None) == ERR_ARG
        # a profile, then d_dynrng: refused, the profile stays and d_compr alone is accepted
        engine.set_encode_drc(2, state)
        with_profile = T.encode(engine, pcm, drc=T.KEEP)
        assert lib.ac3mi_set_encode_dynrng_frames(ctx, ctypes.c_void_p(d.data_ptr()), None) == ERR_ARG
        assert b"profile" in lib.ac3mi_last_error(ctx)
        state.zero_()
        assert np.array_equal(T.encode(engine, pcm, drc=T.KEEP), with_profile), "the refused arrays left the setting unchanged"
        engine.set_encode_dynrng_frames(None, c)
        engine.set_encode_dynrng_frames(None, None)
        engine.set_encode_drc(0)
        # d_dynrng, then a profile: refused, the arrays stay
        engine.set_encode_dynrng_frames(d, c)
        with_arrays = T.encode(engine, pcm, drc=T.KEEP)
        D.check_frames(with_arrays, codes, compr, 7)
        assert lib.ac3mi_set_encode_drc(ctx, 1, ctypes.c_void_p(state.data_ptr())) == ERR_ARG
        assert np.array_equal(T.encode(engine, pcm, drc=T.KEEP), with_arrays)
        engine.set_encode_dynrng_frames(None, None)
        # source mode: dynrng 1 in the decode descriptor, or a profile, is refused at the call
        engine.set_encode_drc_source(1)
        with pytest.raises(H.pkg().AC3MIError, match="twice"):
            _transcode(engine, src, 1536, 7, 1, 7 | 16, 448000, H.CHMAP6, dynrng=1)
        engine.set_encode_drc(1, state)
        with pytest.raises(H.pkg().AC3MIError, match="profile"):
            _transcode(engine, src, 1536, 7, 1, 7 | 16, 448000, H.CHMAP6)
        engine.set_encode_drc(0)
        _transcode(engine, src, 1536, 7, 1, 7 | 16, 448000, H.CHMAP6)
    finally:
        _restore(engine)
    # the workspace grows by the new arrays (40 bytes a frame) in source mode only: a context of its own, which nothing has grown yet
    fresh = H.pkg().Engine(0)
    try:
        fresh.set_encode_dynrng_frames(d, c)
        _transcode(fresh, src, 1536, 7, 1, 7 | 16, 448000, H.CHMAP6)
        mode0 = fresh.workspace_bytes()
        fresh.set_encode_dynrng_frames(None, None)
        fresh.set_encode_drc_source(1)
        _transcode(fresh, src, 1536, 7, 1, 7 | 16, 448000, H.CHMAP6)
        assert fresh.workspace_bytes() == mode0 + 40 * S * F
    finally:
        fresh.close()
