"""GPU: channel coupling in the encoder (ac3mi_set_encode_coupling).  Mode 0 is the reference byte for byte; mode 1 on
content no frame couples is mode 0's bytes; the coupling side information of block 0 is the numpy model's
(tests/coupling_model.py, from the mode-0 taps); every coupled stream decodes cleanly with the liba52 restatement and the
GPU decoder alike; call shapes, block switching, rematrixing, transcode and a large batch."""
import ctypes

import numpy as np
import pytest

from tests import _harness as H
from tests import _tools as T
from tests import block_switch_model as B
from tests import coupling_model as C

pytestmark = pytest.mark.gpu


def _model(t0, nch, begf, sw=None):
    """The model's decisions from the mode-0 taps: [S][F] cplinu, and per frame (mstr, codes) or None."""
    S, F = t0["mdct"].shape[:2]
    nfbw = 5 if nch == 6 else nch
    out = []
    for s in range(S):
        row = []
        for f in range(F):
            switched = sw is not None and bool(sw[s, f, :, :nfbw].any())
            row.append(C.decide(t0["mdct"][s, f], t0["exp_samples"][s, f], nfbw, begf, switched=switched))
        out.append(row)
    return out


def _check_side_info(frames, want, nch, begf):
    nfbw = 5 if nch == 6 else nch
    S, F = frames.shape[:2]
    n_on = 0
    for s in range(S):
        for f in range(F):
            cplinu, chincpl, bf, ef, co = T.coupling_view(frames[s, f], nch)
            w = want[s][f]
            assert cplinu == w[0], (s, f)
            if cplinu:
                n_on += 1
                assert chincpl == (1 << nfbw) - 1 and bf == begf and ef == 12
                assert [m for m, _ in co] == w[1] and [c for _, c in co] == w[2], (s, f)
    return n_on


@pytest.mark.parametrize("nch", [1, 2, 6])
def test_mode0_is_the_reference(engine, nch):
    pcm = np.stack([H.gen_pcm(2, nch, seed=31 + s, kind="music") for s in range(2)])
    want = np.stack([H.orc_encode(p, nch, T.RATE[nch], chmap=(T.chmap_of(nch) + (0,) * 8)[:8]) for p in pcm])
    assert np.array_equal(T.encode(engine, pcm, cpl=(0, 5)), want)
    if nch == 1:                                # one full-bandwidth channel: mode 1 changes nothing
        assert np.array_equal(T.encode(engine, pcm, cpl=(1, 0)), want)


def test_uncoupled_frames_are_mode0(engine):
    pcm = T.content("antiphase", 2, 2, 3, seed=37)
    f0, t0 = T.encode(engine, pcm, cpl=(0, 0), taps=True)
    assert not any(w[0] for row in _model(t0, 2, 0) for w in row)
    assert np.array_equal(T.encode(engine, pcm, cpl=(1, 0)), f0)


@pytest.mark.parametrize("nch", [2, 5, 6])
@pytest.mark.parametrize("pack", [1, 2])
@pytest.mark.parametrize("F", [1, 3])
def test_side_information_matches_the_model(engine, nch, pack, F):
    """(pack 2 asks for the block packer; coupled frames are packed by the one-wavefront packer whatever the mode: the
    uncoupled frames of the pack-2 runs are the block packer's)"""
    engine.set_encode_mode(pack)
    try:
        n_on = 0
        for kind, begf in (("music", 0), ("identical", 3), ("noise", 7), ("music", 12)):
            pcm = T.content(kind, nch, 2, F, seed=43)
            _, t0 = T.encode(engine, pcm, cpl=(0, 0), taps=True)
            frames = T.encode(engine, pcm, cpl=(1, begf))
            n_on += _check_side_info(frames, _model(t0, nch, begf), nch, begf)
            T.decodes_cleanly(frames, *T.layout_of(nch), engine=engine)
        assert n_on > 0
    finally:
        engine.set_encode_mode(0)


def _coords(frames, nch):
    """Per frame: cplinu and, when coupled, the coordinate values [nfbw][nb] (liba52's, x8 included)."""
    out = []
    for s_ in range(frames.shape[0]):
        row = []
        for f in range(frames.shape[1]):
            cplinu, _, _, _, co = T.coupling_view(frames[s_, f], nch)
            row.append((cplinu, None if not cplinu else np.array([[C.coord_value(c, m) for c in cc] for m, cc in co])))
        out.append(row)
    return out


@pytest.mark.parametrize("nch", [2, 6])
def test_decoded_coupling_structure(engine, nch):
    """The GPU decoder (bit-identical to liba52, checked by T.decodes_cleanly) on coupled streams: its coupling-channel taps
    (row 6) are present exactly in the frames the model couples; in coupled bins with bap > 0 channel ch's coefficient
    over channel 0's is the ratio of their decoded coordinates; over the frames, each coupled band's decoded energy per
    channel is within 1.5 dB of the input's (mode-0 MDCT rows c at exp_samples x: c 2^-(23 + x)), as the low band is,
    wherever mode 0's decode is (the top bands of this content sit at the dither floor in both modes)."""
    begf, F, S = 2, 4, 2
    nfbw = 5 if nch == 6 else nch
    pcm = T.content("music", nch, S, F, seed=47)
    _, t0 = T.encode(engine, pcm, cpl=(0, 0), taps=True)
    want = _model(t0, nch, begf)
    frames = T.encode(engine, pcm, cpl=(1, begf))
    T.decodes_cleanly(frames, *T.layout_of(nch), engine=engine)
    _, status, tp = T.decode(engine, frames, *T.layout_of(nch), taps=True)
    f0 = T.encode(engine, pcm, cpl=(0, 0))
    coef0 = T.decode(engine, f0, *T.layout_of(nch), taps=True)[2]["coef"].astype(np.float64)
    # (the decoder's coefficient planes put the LFE first: coded channel ch is plane ch + 1 in 5.1)
    o = 1 if nch == 6 else 0
    coef0 = coef0[:, :, :, o:o + nfbw]
    co = _coords(frames, nch)
    cs, nb = C.start_mant(begf), C.nbands(begf)
    coef = tp["coef"].astype(np.float64)[:, :, :, o:o + nfbw]
    n_on = 0
    e_dec = np.zeros((nfbw, nb + 1))
    e_in = np.zeros((nfbw, nb + 1))
    e_m0 = np.zeros((nfbw, nb + 1))
    for s_ in range(S):
        for f in range(F):
            cplinu = want[s_][f][0]
            assert co[s_][f][0] == cplinu
            assert bool(tp["bap"][s_, f, :, 6].any() or tp["exp"][s_, f, :, 6].any()) == bool(cplinu), (s_, f)
            if not cplinu:
                continue
            n_on += 1
            v = co[s_][f][1]
            bap = tp["bap"][s_, f, :, 6]                                  # [6][256]
            for b in range(6):
                for k in range(cs, 217):
                    if bap[b, k] > 0 and coef[s_, f, b, 0, k] != 0:
                        bd = (k - cs) // 12
                        for ch in range(1, nfbw):
                            want_r = v[ch][bd] / v[0][bd]
                            got_r = coef[s_, f, b, ch, k] / coef[s_, f, b, 0, k]
                            assert abs(got_r - want_r) <= 1e-4 * max(1.0, abs(want_r)), (s_, f, b, ch, k, got_r, want_r)
            x = t0["mdct"][s_, f].astype(np.float64) * np.exp2(-(23.0 + t0["exp_samples"][s_, f]))[..., None]
            for ch in range(nfbw):
                e_dec[ch, nb] += (coef[s_, f, :, ch, 13:cs] ** 2).sum()
                e_in[ch, nb] += (x[:, ch, 13:cs] ** 2).sum()
                for bd in range(nb):
                    lo = cs + 12 * bd
                    e_dec[ch, bd] += (coef[s_, f, :, ch, lo:lo + 12] ** 2).sum()
                    e_in[ch, bd] += (x[:, ch, lo:lo + 12] ** 2).sum()
                    e_m0[ch, bd] += (coef0[s_, f, :, ch, lo:lo + 12] ** 2).sum()
    assert n_on > 0
    db = 10 * np.log10(e_dec / e_in)
    rel = db[:, :nb] - db[:, nb:]
    db0 = 10 * np.log10(e_m0[:, :nb] / e_in[:, :nb])
    print("%d ch: low band %s dB; coupled bands, decoded / input dB:\n%s\nmode 0 decoded / input dB:\n%s" %
          (nch, np.round(db[:, nb], 2).tolist(), np.round(db[:, :nb], 2), np.round(db0, 2)))
    assert np.abs(db[:, nb]).max() < 1.0, db[:, nb]
    # within 1.5 dB of the input wherever mode 0 is (10 of the 13 bands here).  The top bands of this content sit at the
    # decoder's dither floor, where mode 0's own decode misses the input by 2 - 5 dB: there the coupled decode is held only
    # to within 4 dB of mode 0's (measured when written: 0.2 - 3.5 dB below it at 5.1, within 1 dB in stereo)
    held = np.abs(db0) <= 1.5
    assert held.mean() > 0.5 and np.abs(db[:, :nb][held]).max() <= 1.5, np.round(db[:, :nb], 2)
    assert np.abs((db[:, :nb] - db0)[~held]).max(initial=0.0) <= 4.0, np.round(db[:, :nb] - db0, 2)


def test_quality_at_224_kbps(engine):
    """5.1 music at 224 kb/s: 16 csnroffst + fsnroffst rises in every coupled frame (measured when written: +50.8 on average,
    166-220 -> 236-262); stereo music at 96 kb/s decodes better below cplstrtmant (28.07 -> 30.75 dB, +2.68).  The thresholds
    keep half of the offset gain and 1.5 dB of the SNR gain."""
    F = 6
    pcm = T.content("music", 6, 1, F, seed=53)
    f0, t0 = T.encode(engine, pcm, cpl=(0, 0), taps=True, rate=224000)
    f1, t1 = T.encode(engine, pcm, cpl=(1, 0), taps=True, rate=224000)
    on = np.array([T.coupling_view(f1[0, f], 6)[0] for f in range(F)], bool)
    o0 = 16 * t0["snroffst"][0, :, 0] + t0["snroffst"][0, :, 1]
    o1 = 16 * t1["snroffst"][0, :, 0] + t1["snroffst"][0, :, 1]
    print("5.1 224 kb/s: coupled %s, 16 csnr + fsnr %s -> %s (mean +%.1f)" % (on.tolist(), o0.tolist(), o1.tolist(), (o1 - o0)[on].mean()))
    assert on.all() and (o1 > o0).all() and (o1 - o0).mean() >= 25, (o0, o1)
    T.decodes_cleanly(f1, 7, 1, engine=engine)
    # 5.1: the decoded coefficient planes below cplstrtmant against the mode-0 rows (scale fitted on the mode-0 decode)
    x = t0["mdct"][0].astype(np.float64) * np.exp2(-(23.0 + t0["exp_samples"][0]))[..., None]
    x = x[:, :, :5, :C.start_mant(0)]
    d0 = T.decode(engine, f0, 7, 1, taps=True)[2]["coef"][0, :, :, 1:6, :C.start_mant(0)].astype(np.float64)    # (LFE plane first)
    d1 = T.decode(engine, f1, 7, 1, taps=True)[2]["coef"][0, :, :, 1:6, :C.start_mant(0)].astype(np.float64)
    k = (d0 * x).sum() / (x * x).sum()
    snr0 = 10 * np.log10((x ** 2).sum() / ((d0 / k - x) ** 2).sum())
    snr1 = 10 * np.log10((x ** 2).sum() / ((d1 / k - x) ** 2).sum())
    print("5.1 224 kb/s: coefficient SNR below cplstrtmant %.2f -> %.2f dB (+%.2f)" % (snr0, snr1, snr1 - snr0))
    assert snr1 - snr0 >= 1.5, (snr0, snr1)
    # stereo at 96 kb/s, decoded SNR below cplstrtmant (FFT of the error, frame 0 aside)
    pcm2 = T.content("music", 2, 1, F, seed=59)
    cut = C.start_mant(0) * 24000.0 / 256

    def low_snr(frames):
        out, errs, _ = H.orc_decode(frames, 2, 1.0, 0.0)
        assert errs == 0
        dec = out.transpose(0, 1, 3, 2).reshape(-1, 2).astype(np.float64) * 32768.0
        ref = pcm2[0][:dec.shape[0] - 256].astype(np.float64)
        err = dec[256 + 1536:] - ref[1536:]
        E, R = np.fft.rfft(err, axis=0), np.fft.rfft(ref[1536:], axis=0)
        k = np.arange(E.shape[0]) * 24000.0 / (E.shape[0] - 1)
        lo = k < 0.9 * cut
        return 10 * np.log10((np.abs(R[lo]) ** 2).sum() / (np.abs(E[lo]) ** 2).sum())

    s0 = low_snr(T.encode(engine, pcm2, cpl=(0, 0), rate=96000)[0])
    s1 = low_snr(T.encode(engine, pcm2, cpl=(1, 0), rate=96000)[0])
    print("2/0 96 kb/s: decoded SNR below %.0f Hz %.2f -> %.2f dB (+%.2f)" % (cut, s0, s1, s1 - s0))
    assert s1 - s0 >= 1.5, (s0, s1)


def test_call_shapes_agree(engine):
    """Two calls of two frames, state slots, and small tiles give the bytes of one call."""
    import torch
    S, F, nch = 3, 4, 6
    pcm = T.content("music", nch, S, F, seed=61)
    whole = T.encode(engine, pcm, cpl=(1, 1))
    assert any(T.coupling_view(whole[s, f], nch)[0] for s in range(S) for f in range(F))
    last = torch.zeros((S, nch, 256), dtype=torch.int16, device="cuda")
    csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
    a = T.encode(engine, pcm[:, :2 * 1536], cpl=(1, 1), last=last, csnr=csnr)
    b = T.encode(engine, pcm[:, 2 * 1536:], cpl=(1, 1), last=last, csnr=csnr)
    assert np.array_equal(np.concatenate([a, b], 1), whole)
    perm = torch.tensor([2, 0, 1], dtype=torch.int32, device="cuda")
    last6 = torch.zeros((S, 6, 256), dtype=torch.int16, device="cuda")
    csnr6 = torch.full((S,), 40, dtype=torch.int32, device="cuda")
    engine._check(engine.lib.ac3mi_set_state_slots(ctypes.c_void_p(engine.ctx), ctypes.c_void_p(perm.data_ptr())))
    try:
        got = [T.encode(engine, pcm[:, f * 1536:(f + 1) * 1536], cpl=(1, 1), last=last6, csnr=csnr6) for f in range(F)]
    finally:
        engine._check(engine.lib.ac3mi_set_state_slots(ctypes.c_void_p(engine.ctx), None))
    assert np.array_equal(np.concatenate(got, 1), whole)
    engine._check(engine.lib.ac3mi_set_tile_frames(ctypes.c_void_p(engine.ctx), ctypes.c_longlong(4)))
    try:
        tiled = T.encode(engine, pcm, cpl=(1, 1))
    finally:
        engine._check(engine.lib.ac3mi_set_tile_frames(ctypes.c_void_p(engine.ctx), ctypes.c_longlong(0)))
    assert np.array_equal(tiled, whole)


def test_with_block_switching(engine):
    """Frames with a switched block are not coupled, as the model says.  A declined frame 0 is mode 0's frame with block
    switching on byte for byte; a later declined frame may differ from mode 0's through the SNR-offset search, which starts
    from the previous (possibly coupled) frame's offset, so only frame 0 is compared."""
    nch = 2
    pcm = T.content("attack", nch, 2, 4, seed=67)
    f0, t0 = T.encode(engine, pcm, cpl=(0, 0), bsw=1, taps=True)
    sw = np.stack([B.decisions(p, (0, 1), 2) for p in pcm])
    want = _model(t0, nch, 0, sw=sw)
    f1 = T.encode(engine, pcm, cpl=(1, 0), bsw=1)
    on = _check_side_info(f1, want, nch, 0)
    off = [(s, f) for s in range(2) for f in range(4) if not want[s][f][0]]
    assert on > 0 and off
    for s, f in off:
        assert sw[s, f].any()
        if f == 0:
            assert np.array_equal(f1[s, f], f0[s, f])
    T.decodes_cleanly(f1, *T.layout_of(nch), engine=engine)


def test_with_rematrixing(engine):
    """2/0 with rematrixing on: the coupling decision is the model's (rematrixing does not decline a frame); a coupled
    frame's block-0 flags are the mode-1 rule over liba52's cplinu-1 bands (tests/coupling_model.py:remat_coupled), on
    the rows before rematrixing; some frames are both coupled and rematrixed; every stream decodes cleanly."""
    nch = 2
    both = 0
    for kind, begf in (("music", 0), ("music", 1), ("identical", 2), ("music", 5), ("noise", 4)):
        pcm = T.content(kind, nch, 2, 3, seed=71)
        _, t0 = T.encode(engine, pcm, cpl=(0, 0), taps=True)             # rows before rematrixing
        want = _model(t0, nch, begf)
        frames = T.encode(engine, pcm, cpl=(1, begf), remat=1)
        _check_side_info(frames, want, nch, begf)
        for s_ in range(2):
            for f in range(3):
                if not want[s_][f][0]:
                    continue
                rm = []
                T.coupling_view(frames[s_, f], nch, remat=rm)
                fl = C.remat_coupled(t0["mdct"][s_, f], t0["exp_samples"][s_, f], begf)
                assert rm == [1, fl[0]], (kind, begf, s_, f, rm, fl)
                both += fl[0] != 0
        T.decodes_cleanly(frames, *T.layout_of(nch), engine=engine)
    assert both > 0


def test_transcode_equals_decode_then_encode(engine):
    import torch
    pkg = H.pkg()
    S, F, nch = 3, 3, 2
    src = T.encode(engine, T.content("music", nch, S, F, seed=101), cpl=(0, 0))
    fb = src.shape[2]
    stride = (fb + 3) & ~3
    buf = np.zeros((S, F, stride), np.uint8)
    buf[:, :, :fb] = src
    frames_t = torch.from_numpy(buf).cuda()
    dec = pkg.DecodeDesc(flags=2 | 32, level=1.0, bias=384.0, dynrng=1, acmod=2, lfeon=0, frame_bytes=fb)
    enc = pkg.EncodeDesc(48000, 192000, 2)
    engine.set_encode_coupling(1, 2)
    try:
        delay = torch.zeros((S, 2, 128), dtype=torch.float32, device="cuda")
        lfsr = torch.ones((S,), dtype=torch.int16, device="cuda")
        last = torch.zeros((S, 2, 256), dtype=torch.int16, device="cuda")
        csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
        out, status = engine.transcode_batch(dec, enc, frames_t, delay, lfsr, (0, 1), last, csnr)
        engine.sync()
        delay2 = torch.zeros((S, 2, 128), dtype=torch.float32, device="cuda")
        lfsr2 = torch.ones((S,), dtype=torch.int16, device="cuda")
        pcmf, _ = engine.decode_batch(dec, frames_t, delay2, lfsr2)
        s16 = torch.empty((S * F * 6, 256, 2), dtype=torch.int16, device="cuda")
        engine.sync()
        _, oflags = engine.decode_planes(dec)
        engine._check(engine.lib.ac3mi_convert_s16_batch(ctypes.c_void_p(engine.ctx), ctypes.c_void_p(pcmf.data_ptr()),
                                                         ctypes.c_void_p(s16.data_ptr()), oflags, ctypes.c_size_t(S * F * 6)))
        last2 = torch.zeros((S, 2, 256), dtype=torch.int16, device="cuda")
        csnr2 = torch.full((S,), 40, dtype=torch.int32, device="cuda")
        out2 = engine.encode_batch(enc, s16.contiguous().view(S, F, 1536, 2), (0, 1), last2, csnr2)
        engine.sync()
    finally:
        engine.set_encode_coupling(0, 0)
    assert int((status.cpu() & 0x1ff).max()) == 0
    assert torch.equal(out.cpu(), out2.cpu()) and torch.equal(last.cpu(), last2.cpu()) and torch.equal(csnr.cpu(), csnr2.cpu())
    o = out.cpu().numpy()[:, :, :fb]
    assert any(T.coupling_view(o[s, f], 2)[0] for s in range(S) for f in range(F))


def test_large_batch(engine):
    """4 096 one-frame 5.1 streams: every frame passes both CRCs and decodes cleanly."""
    import bench
    S = 4096
    rng = np.random.default_rng(91)
    pool = np.concatenate([T.content(k, 6, 4, 1, seed=92) for k in ("music", "identical", "noise")])
    pcm = np.stack([pool[rng.integers(0, len(pool))] for _ in range(S)])
    pcm = (pcm.astype(np.int32) * rng.uniform(0.3, 1.0, (S, 1, 1))).astype(np.int16)
    frames = T.encode(engine, pcm, cpl=(1, 4))
    assert bench.ac3_crc_ok(frames.reshape(-1, frames.shape[2])) == 0
    on = np.array([T.coupling_view(frames[s, 0], 6)[0] for s in range(0, S, 64)])
    assert 0 < on.mean()
    got, status, _ = T.decode(engine, frames, 7, 1)
    assert (status & 0x1ff).max() == 0
    ref, errs, _ = H.orc_decode(frames[:64, 0], 7 | 16, 1.0, 0.0)     # (64 frames as one stream: each frame stands alone)
    assert errs == 0


def test_setter_rejects_bad_arguments(engine):
    for mode, begf in ((-1, 0), (2, 0), (1, -1), (1, 13), (0, 13)):
        with pytest.raises(Exception):
            engine.set_encode_coupling(mode, begf)
    engine.set_encode_coupling(0, 0)
