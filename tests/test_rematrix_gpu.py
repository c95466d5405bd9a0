"""GPU: stereo rematrixing in the encoder (ac3mi_set_encode_rematrix).  Off, and on for other layouts or for stereo where no
band qualifies, is the reference byte for byte; on, the coded rows equal the numpy model's (tests/rematrix_model.py) on the
mode-0 rows, the flags in the bitstream are the model's, every frame decodes cleanly with the liba52 restatement and the
GPU decoder alike, and correlated stereo gets a higher SNR offset and a better decode."""
import ctypes

import numpy as np
import pytest

from tests import _harness as H
from tests import _tools as T
from tests import block_switch_model as B
from tests import rematrix_model as M

pytestmark = pytest.mark.gpu


def _expect(engine, pcm, bsw=0, lasts=None):
    """The model's mode-1 rows, shifts, flags and rematstr [S][F][6]... from the mode-0 taps of the same content."""
    import torch
    last0 = None if lasts is None else torch.from_numpy(np.ascontiguousarray(lasts)).cuda()
    _, t0 = T.encode(engine, pcm, remat=0, bsw=bsw, taps=True, last=last0)
    want = []
    for s in range(pcm.shape[0]):
        last = None if lasts is None else lasts[s]
        v = M.block_v(pcm[s], (0, 1), last)
        assert np.array_equal(v - 9, t0["exp_samples"][s]), "v of the model != the encoder's block shift"
        sw = B.decisions(pcm[s], (0, 1), 2, last) if bsw else None
        want.append(M.rematrix(t0["mdct"][s], v, sw))
    return [np.stack([w[i] for w in want]) for i in range(4)], t0


def _check_rows(engine, pcm, bsw=0, lasts=None):
    (rows, shift, flags, rs), _ = _expect(engine, pcm, bsw, lasts=lasts)
    frames, t1 = T.encode(engine, pcm, remat=1, bsw=bsw, taps=True)
    assert np.array_equal(t1["mdct"], rows), np.argwhere(t1["mdct"] != rows)[:8]
    assert np.array_equal(t1["exp_samples"], shift)
    return frames, flags, rs


@pytest.mark.parametrize("nch", [1, 2, 6])
def test_off_and_non_stereo_are_the_reference(engine, nch):
    for kind in ("tones", "music"):
        pcm = np.stack([H.gen_pcm(2, nch, seed=31 + s, kind=kind) for s in range(2)])
        want = np.stack([H.orc_encode(p, nch, T.RATE[nch], chmap=(T.chmap_of(nch) + (0,) * 8)[:8]) for p in pcm])
        assert np.array_equal(T.encode(engine, pcm, remat=0), want), kind
        if nch != 2:
            assert np.array_equal(T.encode(engine, pcm, remat=1), want), kind
        assert np.array_equal(T.encode(engine, pcm, remat=0), want), kind


@pytest.mark.parametrize("kind", ["quietR", "silentR"])
def test_no_qualifying_band_is_the_reference(engine, kind):
    pcm = T.stereo(kind, 2, 3, seed=41)
    (_, _, flags, _), _ = _expect(engine, pcm)
    assert flags.sum() == 0
    want = np.stack([H.orc_encode(p, 2, T.RATE[2], chmap=(0, 1) + (0,) * 6) for p in pcm])
    assert np.array_equal(T.encode(engine, pcm, remat=1), want)


@pytest.mark.parametrize("pack", [1, 2])
@pytest.mark.parametrize("F", [1, 3])
def test_rows_equal_the_model(engine, pack, F):
    engine.set_encode_mode(pack)
    try:
        for kind in ("tones", "noise", "identical", "nearmono", "changing"):
            pcm = T.stereo(kind, 3, F, seed=51)
            frames, flags, rs = _check_rows(engine, pcm)
            if kind in ("identical", "nearmono"):
                assert flags.min() == 15, kind
            if kind == "changing" and F == 3:
                assert 0 < flags.astype(bool).mean() < 1 and rs[:, :, 1:].sum() > 0
            got_rs, got_fl = T.remat_view(frames)
            assert np.array_equal(got_rs, np.ones_like(got_rs)) and np.array_equal(got_fl, flags[:, :, 0]), kind
    finally:
        engine.set_encode_mode(0)


@pytest.mark.parametrize("pack", [1, 2])
def test_rows_with_block_switching(engine, pack):
    engine.set_encode_mode(pack)
    try:
        pcm = T.stereo("attack", 3, 3, seed=57)
        sw = np.stack([B.decisions(p, (0, 1), 2) for p in pcm])
        assert (sw[..., 0] != sw[..., 1]).any() and (sw[..., 0] & sw[..., 1]).any()
        frames, flags, _ = _check_rows(engine, pcm, bsw=1)
        assert flags[sw[..., 0] != sw[..., 1]].sum() == 0 and flags.sum() > 0
        _check_rows(engine, pcm, bsw=0)
    finally:
        engine.set_encode_mode(0)


def test_split_call_and_state_slots(engine):
    """Two calls of two frames each give the bytes of one call of four; so do state slots in a permuted order."""
    import torch
    S, F = 3, 4
    pcm = T.stereo("changing", S, F, seed=61)
    whole, flags, _ = _check_rows(engine, pcm)
    assert flags.sum() > 0
    last = torch.zeros((S, 2, 256), dtype=torch.int16, device="cuda")
    csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
    a = T.encode(engine, pcm[:, :2 * 1536], remat=1, last=last, csnr=csnr)
    lasts = last.cpu().numpy()
    b, t = T.encode(engine, pcm[:, 2 * 1536:], remat=1, last=last, csnr=csnr, taps=True)
    assert np.array_equal(np.concatenate([a, b], 1), whole)
    # the second call's rows against the model with the history the first call left
    (rows, _, _, _), _ = _expect(engine, pcm[:, 2 * 1536:], lasts=lasts)
    assert np.array_equal(t["mdct"], rows)
    perm = torch.tensor([2, 0, 1], dtype=torch.int32, device="cuda")
    last6 = torch.zeros((S, 6, 256), dtype=torch.int16, device="cuda")
    csnr6 = torch.full((S,), 40, dtype=torch.int32, device="cuda")
    engine._check(engine.lib.ac3mi_set_state_slots(ctypes.c_void_p(engine.ctx), ctypes.c_void_p(perm.data_ptr())))
    try:
        got = []
        for f in range(F):
            got.append(T.encode(engine, pcm[:, f * 1536:(f + 1) * 1536], remat=1,
                               last=last6.view(-1)[:S * 2 * 256].view(S, 2, 256), csnr=csnr6))
    finally:
        engine._check(engine.lib.ac3mi_set_state_slots(ctypes.c_void_p(engine.ctx), None))
    assert np.array_equal(np.concatenate(got, 1), whole)


def test_rematrixed_streams_decode_like_liba52(engine):
    import bench
    pcm = np.concatenate([T.stereo(k, 1, 3, seed=71) for k in ("identical", "nearmono", "changing", "tones")])
    for bsw in (0, 1):
        frames = T.encode(engine, pcm, remat=1, bsw=bsw)
        assert bench.ac3_crc_ok(frames.reshape(-1, frames.shape[2])) == 0
        got, status, _ = T.decode(engine, frames, 2, 0)
        assert (status & 0x1ff).max() == 0
        for s in range(pcm.shape[0]):
            ref, errs, _ = H.orc_decode(frames[s], 2, 1.0, 0.0)
            assert errs == 0
            err = got[s].astype(np.float64) - ref.reshape(got[s].shape)
            assert H.rms(err) <= 1e-6, H.rms(err)


def _decoded_snr(frames, pcm):
    out, errs, _ = H.orc_decode(frames, 2, 1.0, 0.0)
    assert errs == 0
    dec = out.transpose(0, 1, 3, 2).reshape(-1, 2).astype(np.float64) * 32768.0
    ref = pcm[:dec.shape[0] - 256].astype(np.float64)
    err = dec[256 + 1536:] - ref[1536:]                     # (frame 0 starts from a zero history)
    return 10 * np.log10((ref[1536:] ** 2).sum() / (err ** 2).sum())


def test_quality_gain(engine):
    """At 96 kb/s the mode-0 search does not saturate (csnroffst < 63): correlated stereo gets a strictly higher
    16 csnroffst + fsnroffst in every frame and a better decode.  Measured over 6 frames of the harness's music: identical
    L/R +38.3 on average (166-201 -> 204-228), decoded SNR 25.8 -> 30.3 dB (+4.5); near-mono +30.8, 25.8 -> 29.4 dB (+3.7).
    The thresholds keep half of the smaller gain in hand."""
    F = 6
    for kind in ("music_identical", "music_nearmono"):
        pcm = T.stereo(kind, 1, F, seed=81)
        f0, t0 = T.encode(engine, pcm, remat=0, taps=True, rate=96000)
        f1, t1 = T.encode(engine, pcm, remat=1, taps=True, rate=96000)
        o0 = 16 * t0["snroffst"][0, :, 0] + t0["snroffst"][0, :, 1]
        o1 = 16 * t1["snroffst"][0, :, 0] + t1["snroffst"][0, :, 1]
        assert t0["snroffst"][0, :, 0].max() < 63
        snr0, snr1 = _decoded_snr(f0[0], pcm[0]), _decoded_snr(f1[0], pcm[0])
        print("%s: 16 csnr + fsnr %s -> %s (mean +%.1f), decoded SNR %.2f -> %.2f dB (+%.2f)" %
              (kind, o0.tolist(), o1.tolist(), (o1 - o0).mean(), snr0, snr1, snr1 - snr0))
        assert (o1 > o0).all() and (o1 - o0).mean() >= 15, (o0, o1)
        assert snr1 - snr0 >= 2.0, (snr0, snr1)


def test_large_batch(engine):
    """4 096 one-frame streams: the one-wavefront packer and the remapped grid; rows equal the model's."""
    S = 4096
    rng = np.random.default_rng(91)
    kinds = ("identical", "nearmono", "changing", "noise", "tones")
    pools = {k: T.stereo(k, 8, 1, seed=92) for k in kinds}
    pcm = np.stack([pools[kinds[i % 5]][rng.integers(0, 8)] for i in range(S)])
    pcm = (pcm.astype(np.int32) * rng.uniform(0.3, 1.0, (S, 1, 1))).astype(np.int16)
    frames, flags, _ = _check_rows(engine, pcm)
    assert 0 < flags.astype(bool).mean() < 1
    import bench
    assert bench.ac3_crc_ok(frames.reshape(-1, frames.shape[2])) == 0


def test_transcode_equals_decode_then_encode(engine):
    """ac3mi_transcode_batch with rematrixing (2/0 in, stereo out) == decode_batch + convert_s16_batch + encode_batch
    with it, byte for byte and state for state."""
    import torch
    pkg = H.pkg()
    S, F = 3, 3
    src = T.encode(engine, np.concatenate([T.stereo(k, 1, F, seed=101) for k in ("nearmono", "changing", "tones")]), remat=1)
    fb = src.shape[2]
    stride = (fb + 3) & ~3
    buf = np.zeros((S, F, stride), np.uint8)
    buf[:, :, :fb] = src
    frames_t = torch.from_numpy(buf).cuda()
    dec = pkg.DecodeDesc(flags=2 | 32, level=1.0, bias=384.0, dynrng=1, acmod=2, lfeon=0, frame_bytes=fb)
    enc = pkg.EncodeDesc(48000, 192000, 2)
    engine.set_encode_rematrix(1)
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
        engine.set_encode_rematrix(0)
    assert int((status.cpu() & 0x1ff).max()) == 0
    assert torch.equal(out.cpu(), out2.cpu()) and torch.equal(last.cpu(), last2.cpu()) and torch.equal(csnr.cpu(), csnr2.cpu())
    assert T.remat_view(out.cpu().numpy()[:, :, :fb])[1].sum() > 0


def test_setter_rejects_other_modes(engine):
    pcm = T.stereo("nearmono", 1, 2, seed=111)
    on = T.encode(engine, pcm, remat=1)
    off = T.encode(engine, pcm, remat=0)
    assert not np.array_equal(on, off)
    engine.set_encode_rematrix(1)
    try:
        for m in (-1, 2):
            with pytest.raises(Exception):
                engine.set_encode_rematrix(m)
        assert np.array_equal(T.encode(engine, pcm, remat=T.KEEP), on)        # still mode 1
    finally:
        engine.set_encode_rematrix(0)
    assert np.array_equal(T.encode(engine, pcm, remat=T.KEEP), off)
