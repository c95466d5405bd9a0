"""GPU: encoder metadata (ac3mi_set_encode_metadata) and dynamic range control (ac3mi_set_encode_drc).  Both off leave every
byte as it was after any sequence of settings; metadata reaches the BSI and nothing else, and cmixlev changes what the
decoders downmix; the dynrng words are the numpy model's (tests/drc_model.py) in exactly the blocks it says, for every
profile and three dialnorms; call shapes, transcode, the decoded gain, a large batch and the setters' validation."""
import ctypes

import numpy as np
import pytest

from tests import _harness as H
from tests import _tools as T
from tests import drc_model as D

pytestmark = pytest.mark.gpu

TOOLS_ON = dict(bsw=1, remat=1, cpl=(1, 3), bw=(1, 40))
META = dict(dialnorm=17, bsmod=3, cmixlev=2, surmixlev=0, dsurmod=2, copyrightb=1, origbs=0)


def _model(pcm, nch, profile, dialnorm=31, state=0):
    return D.encode(pcm, T.chmap_of(nch), min(nch, 5), profile, dialnorm, state)


@pytest.mark.parametrize("nch", [1, 2, 6])
@pytest.mark.parametrize("tools", [False, True])
def test_off_means_unchanged(engine, nch, tools):
    """DRC 0 and metadata NULL after any set / reset sequence: a fresh engine's bytes."""
    import torch
    pkg = H.pkg()
    pcm = np.stack([H.gen_pcm(2, nch, seed=71 + s, kind="music") for s in range(2)])
    fresh = pkg.Engine(0)
    try:
        want = T.encode(fresh, pcm, **(TOOLS_ON if tools else {}))
    finally:
        fresh.close()
    if not tools:
        ref = np.stack([H.orc_encode(p, nch, T.RATE[nch], chmap=(T.chmap_of(nch) + (0,) * 8)[:8]) for p in pcm])
        assert np.array_equal(want, ref)
    state = torch.zeros((2,), dtype=torch.int32, device="cuda")
    assert not np.array_equal(T.encode(engine, pcm, drc=2, state=state, md=META, **(TOOLS_ON if tools else {})), want)
    assert np.array_equal(T.encode(engine, pcm, **(TOOLS_ON if tools else {})), want)
    engine.set_encode_metadata(**META)
    engine.set_encode_drc(4, state)
    engine.set_encode_drc(0, state)                 # profile 0 with a state: accepted, sends nothing
    engine.set_encode_metadata()
    try:
        assert np.array_equal(T.encode(engine, pcm, drc=0, md=None, **(TOOLS_ON if tools else {})), want)
        engine.set_encode_metadata(dialnorm=31, bsmod=0, cmixlev=1, surmixlev=1, dsurmod=0, copyrightb=0, origbs=1)
        assert np.array_equal(T.encode(engine, pcm, md=dict(dialnorm=31), **(TOOLS_ON if tools else {})), want)
    finally:
        engine.set_encode_metadata()
        engine.set_encode_drc(0)


@pytest.mark.parametrize("nch", [1, 2, 6])
@pytest.mark.parametrize("pack", [1, 2])
def test_metadata_reaches_the_bsi_only(engine, nch, pack):
    pcm = np.stack([H.gen_pcm(3, nch, seed=81 + s, kind="music") for s in range(2)])
    engine.set_encode_mode(pack)
    try:
        want = T.encode(engine, pcm)
        got = T.encode(engine, pcm, md=META)
    finally:
        engine.set_encode_mode(0)
    T.decodes_cleanly(got, *T.layout_of(nch), engine=engine)
    acmod = T.ACMOD[nch]
    for s in range(got.shape[0]):
        for f in range(got.shape[1]):
            fields, where = T.bsi_view(got[s, f])
            dflt, where0 = T.bsi_view(want[s, f])
            assert where == where0
            assert fields["dialnorm"] == 17 and fields["bsmod"] == 3 and fields["copyrightb"] == 1 and fields["origbs"] == 0
            assert dflt["dialnorm"] == 31 and dflt["bsmod"] == 0 and dflt["copyrightb"] == 0 and dflt["origbs"] == 1
            assert fields.get("cmixlev") == (2 if (acmod & 1) and acmod != 1 else None)
            assert fields.get("surmixlev") == (0 if acmod & 4 else None)
            assert fields.get("dsurmod") == (2 if acmod == 2 else None)
            assert fields["compre"] == 0 and fields["addbsie"] == 0
            a = np.unpackbits(got[s, f])
            b = np.unpackbits(want[s, f])
            keep = np.ones(a.size, bool)
            keep[list(where)] = False
            keep[16:32] = False                         # crc1
            keep[-16:] = False                          # crc2
            assert np.array_equal(a[keep], b[keep])


def test_downmix_levels(engine):
    """A 3/2 stream with cmixlev 0 (-3 dB) and 2 (-6 dB) decodes to different stereo; the GPU decoder matches the oracle."""
    nch = 6
    pcm = np.stack([H.gen_pcm(2, nch, seed=91, kind="music")])
    outs = []
    for c in (0, 2):
        frames = T.encode(engine, pcm, md=dict(cmixlev=c, surmixlev=c))
        got, status, _ = T.decode(engine, frames, 7, 1, 2)
        assert (status & 0x1ff).max() == 0
        ref, errs, _ = H.orc_decode(frames[0], 2, 1.0, 0.0)
        assert errs == 0
        assert H.rms(got[0].astype(np.float64) - ref.reshape(got[0].shape)) <= 1e-6
        outs.append(got[0].astype(np.float64))
    assert H.rms(outs[0] - outs[1]) > 1e-3


@pytest.mark.parametrize("profile", [1, 2, 3, 4, 5])
def test_codes_match_the_model(engine, profile):
    import torch
    nch = 2
    pcm = T.programme(nch, seed=profile)
    seen = []
    for dialnorm in (31, 24, 1):
        state = torch.zeros((1,), dtype=torch.int32, device="cuda")
        frames = T.encode(engine, pcm, drc=profile, state=state, md=dict(dialnorm=dialnorm))
        codes, snt, s_end, _ = _model(pcm[0], nch, profile, dialnorm)
        assert int(state.cpu()[0]) == s_end
        _, status, taps = T.decode(engine, frames, 2, 0, 2, taps=True)
        assert (status & 0x1ff).max() == 0
        w = taps["dynrng"][0, :, :, 0]
        assert np.array_equal(~np.isnan(w), snt), (dialnorm, snt, w)
        want = np.array([[D.decoded_gain(v) for v in row] for row in codes], np.float32)
        assert np.array_equal(w[snt], want[snt]), dialnorm
        assert all(T.bsi_view(fr)[0]["dialnorm"] == dialnorm for fr in frames[0])
        seen.append(codes)
    # the programme exercises boost and cut (at dialnorm 31, the loud segments sit far above the dialogue level)
    assert seen[0].max() > 0 and seen[0].min() < 0


def test_call_shapes_agree(engine):
    """One call of 12 frames, 12 calls of one frame carrying the state, permuted state slots, a tile bound of 3 frames
    and both packers: the same bytes and final state."""
    import torch
    S, F, nch, prof = 3, 12, 6, 1
    pcm = np.concatenate([T.programme(nch, seed=7 + s) for s in range(S)])
    md = dict(dialnorm=24)

    def fresh():
        return (torch.zeros((S,), dtype=torch.int32, device="cuda"), torch.zeros((S, nch, 256), dtype=torch.int16, device="cuda"),
                torch.full((S,), 40, dtype=torch.int32, device="cuda"))

    st, last, csnr = fresh()
    whole = T.encode(engine, pcm, drc=prof, state=st, md=md, last=last, csnr=csnr)
    st_whole = st.cpu().numpy().copy()
    for s in range(S):
        codes, snt, s_end, _ = _model(pcm[s], nch, prof, 24)
        assert st_whole[s] == s_end
    for pack in (1, 2):
        engine.set_encode_mode(pack)
        try:
            st, last, csnr = fresh()
            assert np.array_equal(T.encode(engine, pcm, drc=prof, state=st, md=md, last=last, csnr=csnr), whole), pack
            assert np.array_equal(st.cpu().numpy(), st_whole)
        finally:
            engine.set_encode_mode(0)
    st, last, csnr = fresh()
    got = [T.encode(engine, pcm[:, f * 1536:(f + 1) * 1536], drc=prof, state=st, md=md, last=last, csnr=csnr) for f in range(F)]
    assert np.array_equal(np.concatenate(got, 1), whole)
    assert np.array_equal(st.cpu().numpy(), st_whole)
    perm = torch.tensor([2, 0, 1], dtype=torch.int32, device="cuda")
    st, last, csnr = fresh()
    engine._check(engine.lib.ac3mi_set_state_slots(ctypes.c_void_p(engine.ctx), ctypes.c_void_p(perm.data_ptr())))
    try:
        got = [T.encode(engine, pcm[:, f * 1536:(f + 1) * 1536], drc=prof, state=st, md=md, last=last, csnr=csnr)
               for f in range(F)]
    finally:
        engine._check(engine.lib.ac3mi_set_state_slots(ctypes.c_void_p(engine.ctx), None))
    assert np.array_equal(np.concatenate(got, 1), whole)
    assert np.array_equal(st.cpu().numpy()[perm.cpu().numpy()], st_whole)
    engine._check(engine.lib.ac3mi_set_tile_frames(ctypes.c_void_p(engine.ctx), ctypes.c_longlong(3)))
    try:
        st, last, csnr = fresh()
        tiled = T.encode(engine, pcm, drc=prof, state=st, md=md, last=last, csnr=csnr)
    finally:
        engine._check(engine.lib.ac3mi_set_tile_frames(ctypes.c_void_p(engine.ctx), ctypes.c_longlong(0)))
    assert np.array_equal(tiled, whole)
    assert np.array_equal(st.cpu().numpy(), st_whole)
    T.decodes_cleanly(whole, *T.layout_of(nch), engine=engine)


def test_drc_with_every_tool(engine):
    """Block switching, rematrixing, coupling and bandwidth on: clean decodes, the model's words (2/0 and 5.1)."""
    import torch
    for nch in (2, 6):
        pcm = T.programme(nch, seed=11)
        st = torch.zeros((1,), dtype=torch.int32, device="cuda")
        frames = T.encode(engine, pcm, drc=3, state=st, md=dict(dialnorm=20), **TOOLS_ON)
        T.decodes_cleanly(frames, *T.layout_of(nch), engine=engine)
        codes, snt, s_end, _ = _model(pcm[0], nch, 3, 20)
        _, status, taps = T.decode(engine, frames, *T.layout_of(nch), taps=True)
        w = taps["dynrng"][0, :, :, 0]
        assert np.array_equal(~np.isnan(w), snt)
        assert int(st.cpu()[0]) == s_end


def test_transcode_equals_decode_then_encode(engine):
    """Transcode with DRC = decode, s16 conversion, encode with DRC: the same frames and final DRC state, in one piece and
    with a tile bound of 4 frames (below S x F: tiles of one stream, each carrying its own stream's DRC state)."""
    for tile in (None, 4):
        _transcode_equals_decode_then_encode(engine, tile)


def _transcode_equals_decode_then_encode(engine, tile):
    import torch
    pkg = H.pkg()
    S, F, nch = 2, 4, 2
    src = T.encode(engine, T.content("music", nch, S, F, seed=121))
    fb = src.shape[2]
    buf = np.zeros((S, F, (fb + 3) & ~3), np.uint8)
    buf[:, :, :fb] = src
    frames_t = torch.from_numpy(buf).cuda()
    dec = pkg.DecodeDesc(flags=2 | 32, level=1.0, bias=384.0, dynrng=1, acmod=2, lfeon=0, frame_bytes=fb)
    enc = pkg.EncodeDesc(48000, 192000, 2)
    st = torch.full((S,), 100, dtype=torch.int32, device="cuda")
    st2 = st.clone()
    engine.set_encode_metadata(dialnorm=27, bsmod=1)
    engine.set_encode_drc(5, st)
    try:
        delay = torch.zeros((S, 2, 128), dtype=torch.float32, device="cuda")
        lfsr = torch.ones((S,), dtype=torch.int16, device="cuda")
        last = torch.zeros((S, 2, 256), dtype=torch.int16, device="cuda")
        csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
        if tile:
            engine.set_tile_frames(tile)
        try:
            out, status = engine.transcode_batch(dec, enc, frames_t, delay, lfsr, (0, 1), last, csnr)
            engine.sync()
        finally:
            engine.set_tile_frames(131072)
        delay2 = torch.zeros((S, 2, 128), dtype=torch.float32, device="cuda")
        lfsr2 = torch.ones((S,), dtype=torch.int16, device="cuda")
        pcmf, _ = engine.decode_batch(dec, frames_t, delay2, lfsr2)
        s16 = torch.empty((S * F * 6, 256, 2), dtype=torch.int16, device="cuda")
        engine.sync()
        _, oflags = engine.decode_planes(dec)
        engine._check(engine.lib.ac3mi_convert_s16_batch(ctypes.c_void_p(engine.ctx), ctypes.c_void_p(pcmf.data_ptr()),
                                                         ctypes.c_void_p(s16.data_ptr()), oflags, ctypes.c_size_t(S * F * 6)))
        engine.set_encode_drc(5, st2)
        last2 = torch.zeros((S, 2, 256), dtype=torch.int16, device="cuda")
        csnr2 = torch.full((S,), 40, dtype=torch.int32, device="cuda")
        out2 = engine.encode_batch(enc, s16.contiguous().view(S, F, 1536, 2), (0, 1), last2, csnr2)
        engine.sync()
    finally:
        engine.set_encode_metadata()
        engine.set_encode_drc(0)
    assert int((status.cpu() & 0x1ff).max()) == 0
    assert torch.equal(out.cpu(), out2.cpu()) and torch.equal(st.cpu(), st2.cpu()) and torch.equal(csnr.cpu(), csnr2.cpu())
    o = out.cpu().numpy()[:, :, :fb]
    T.decodes_cleanly(o, 2, 0, engine=engine)
    x = s16.cpu().numpy().reshape(S, F * 1536, 2)
    for s in range(S):
        codes, snt, s_end, _ = _model(x[s], 2, 5, 27, state=100)
        assert int(st.cpu()[s]) == s_end


def test_workspace_bytes_counts_the_drc_workspace():
    """ac3mi_workspace_bytes includes the DRC workspace (18 bytes a frame): two fresh engines run the same encode call,
    one with DRC profile 1 and one without, and hold exactly that much apart."""
    import torch
    pkg = H.pkg()
    S, F, nch = 3, 4, 2
    pcm = T.content("music", nch, S, F, seed=5)
    held = []
    for drc in (0, 1):
        eng = pkg.Engine(0)
        try:
            state = torch.zeros((S,), dtype=torch.int32, device="cuda")
            T.encode(eng, pcm, drc=drc, state=state)
            held.append(eng.workspace_bytes())
        finally:
            eng.close()
    assert held[1] - held[0] == 18 * S * F, held


def test_decoded_gain_follows_the_model(engine):
    """Per block, decoded RMS with DRC on over DRC off = the model's gain within 0.5 dB, where the gain holds over the
    block and the one before (the overlap-add mixes two blocks' gains)."""
    import torch
    nch = 2
    pcm = T.programme(nch, seed=3)
    off = T.encode(engine, pcm)
    st = torch.zeros((1,), dtype=torch.int32, device="cuda")
    on = T.encode(engine, pcm, drc=1, state=st)
    codes, _, _, _ = _model(pcm[0], nch, 1)
    a, sa, _ = T.decode(engine, off, 2, 0, 2)
    b, sb, _ = T.decode(engine, on, 2, 0, 2)
    assert (sa & 0x1ff).max() == 0 and (sb & 0x1ff).max() == 0
    a = a[0].reshape(-1, 2, 256).astype(np.float64)             # [F * 6][n_out][256]
    b = b[0].reshape(-1, 2, 256).astype(np.float64)
    c = codes.reshape(-1)
    n = 0
    for k in range(2, c.size):
        ra = np.sqrt((a[k] ** 2).mean())
        if c[k] != c[k - 1] or c[k - 1] != c[k - 2] or ra < 1e-3:
            continue
        rb = np.sqrt((b[k] ** 2).mean())
        assert abs(20 * np.log10(rb / ra) - 20 * np.log10(D.decoded_gain(c[k]))) <= 0.5, k
        n += 1
    assert n >= 10


def test_large_batch(engine):
    """65 536 one-frame 5.1 streams under profile 1: every frame decodes clean, a sample carries the model's words."""
    import torch
    pkg = H.pkg()
    N, nch = 65536, 6
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(5)
    t = torch.arange(1536, device=dev, dtype=torch.float32)
    amp = 10 ** (-torch.rand((N, 1, 1), device=dev, generator=g) * 3.5) * 30000
    pcm = amp * torch.sin(0.05 * t[None, :, None] * (1 + torch.rand((N, 1, nch), device=dev, generator=g)))
    pcm = (pcm + (torch.rand((N, 1536, nch), device=dev, generator=g) - 0.5) * 64).round().clamp(-32768, 32767).to(torch.int16)
    enc = pkg.EncodeDesc(48000, 384000, nch)
    st = torch.zeros((N,), dtype=torch.int32, device="cuda")
    last = torch.zeros((N, nch, 256), dtype=torch.int16, device="cuda")
    csnr = torch.full((N,), 40, dtype=torch.int32, device="cuda")
    engine.set_encode_drc(1, st)
    try:
        frames = engine.encode_batch(enc, pcm.view(N, 1, 1536, nch).contiguous(), H.CHMAP6, last, csnr)
        engine.sync()
    finally:
        engine.set_encode_drc(0)
    fb = enc.frame_bytes()
    dec = pkg.DecodeDesc(flags=7 | 16, level=1.0, bias=0.0, dynrng=1, acmod=7, lfeon=1, frame_bytes=fb)
    delay = torch.zeros((N, 6, 128), dtype=torch.float32, device="cuda")
    lfsr = torch.ones((N,), dtype=torch.int16, device="cuda")
    _, status = engine.decode_batch(dec, frames, delay, lfsr)
    engine.sync()
    assert int((status.cpu() & 0x1ff).max()) == 0
    del delay
    sample = np.random.default_rng(1).choice(N, 24, replace=False)
    fr = frames.cpu().numpy()[sample, :, :fb]
    _, status, taps = T.decode(engine, fr, 7, 1, 7 | 16, taps=True)
    assert (status & 0x1ff).max() == 0
    x = pcm.cpu().numpy()[sample]
    stc = st.cpu().numpy()
    for i, s in enumerate(sample):
        codes, snt, s_end, _ = _model(x[i], nch, 1)
        w = taps["dynrng"][i, :, :, 0]
        assert np.array_equal(~np.isnan(w), snt)
        want = np.array([[D.decoded_gain(v) for v in row] for row in codes], np.float32)
        assert np.array_equal(w[snt], want[snt])
        assert stc[s] == s_end


def test_setter_validation(engine):
    import torch
    lib, ctx = engine.lib, ctypes.c_void_p(engine.ctx)
    st = torch.zeros((4,), dtype=torch.int32, device="cuda")
    p = ctypes.c_void_p(st.data_ptr())
    for prof in (-1, 6, 100):
        assert lib.ac3mi_set_encode_drc(ctx, prof, p) != 0
    for prof in (1, 2, 3, 4, 5):
        assert lib.ac3mi_set_encode_drc(ctx, prof, None) != 0
        assert lib.ac3mi_set_encode_drc(ctx, prof, p) == 0
    assert lib.ac3mi_set_encode_drc(ctx, 0, None) == 0
    assert lib.ac3mi_set_encode_drc(None, 0, None) != 0
    good = [31, 0, 1, 1, 0, 0, 1]
    bad = {0: (0, 32, -1), 1: (-1, 8), 2: (3, -1), 3: (3, -1), 4: (3, -1), 5: (2, -1), 6: (2, -1)}
    for i, vals in bad.items():
        for v in vals:
            f = list(good)
            f[i] = v
            md = (ctypes.c_int * 7)(*f)
            assert lib.ac3mi_set_encode_metadata(ctx, ctypes.cast(md, ctypes.c_void_p)) != 0, (i, v)
    for f in ([1, 7, 0, 2, 2, 1, 0], good):
        md = (ctypes.c_int * 7)(*f)
        assert lib.ac3mi_set_encode_metadata(ctx, ctypes.cast(md, ctypes.c_void_p)) == 0
    assert lib.ac3mi_set_encode_metadata(ctx, None) == 0
    assert lib.ac3mi_set_encode_metadata(None, None) != 0
    with pytest.raises(Exception):
        engine.set_encode_metadata(cmixlev=3)
    with pytest.raises(Exception):
        engine.set_encode_drc(2)
    with pytest.raises(TypeError):
        engine.set_encode_metadata(loudness=1)
    engine.set_encode_metadata()
    engine.set_encode_drc(0)
