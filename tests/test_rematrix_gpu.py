"""GPU: stereo rematrixing in the encoder (ac3mi_set_encode_rematrix).  Off, and on for other layouts or for stereo where no
band qualifies, is the reference byte for byte; on, the coded rows equal the numpy model's (tests/rematrix_model.py) on the
mode-0 rows, the flags in the bitstream are the model's, every frame decodes cleanly with the liba52 restatement and the
GPU decoder alike, and correlated stereo gets a higher SNR offset and a better decode."""
import ctypes

import numpy as np
import pytest

from tests import _harness as H
from tests import block_switch_model as B
from tests import rematrix_model as M

pytestmark = pytest.mark.gpu

RATE = {1: 192000, 2: 192000, 6: 384000}


def _chmap(nch):
    return H.CHMAP6 if nch == 6 else tuple(range(nch))


def _encode(engine, pcm, nch, remat, bsw=0, taps=False, last=None, csnr=None, rate=None):
    """pcm [S][F*1536][nch] s16 -> frames [S][F][fb] (numpy)[, taps] with rematrixing `remat` (None: leave the context's
    setting as it is) and block switching `bsw`, one call."""
    import torch
    pkg = H.pkg()
    S = pcm.shape[0]
    F = pcm.shape[1] // 1536
    enc = pkg.EncodeDesc(48000, rate or RATE[nch], nch)
    if last is None:
        last = torch.zeros((S, nch, 256), dtype=torch.int16, device="cuda")
    if csnr is None:
        csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
    if remat is not None:
        engine.set_encode_rematrix(remat)
    engine.set_encode_block_switch(bsw)
    try:
        r = engine.encode_batch(enc, torch.from_numpy(np.ascontiguousarray(pcm).reshape(S, F, 1536, nch)).cuda(), _chmap(nch),
                                last, csnr, taps=taps)
        engine.sync()
    finally:
        if remat is not None:
            engine.set_encode_rematrix(0)
        engine.set_encode_block_switch(0)
    fb = enc.frame_bytes()
    if taps:
        return r[0].cpu().numpy()[:, :, :fb], {k: v.cpu().numpy() for k, v in r[1].items()}
    return r.cpu().numpy()[:, :, :fb]


def _stereo(kind, S, F, seed):
    """[S][F*1536][2] s16 stereo test content."""
    n = F * 1536
    t = np.arange(n)
    out = []
    for s in range(S):
        rng = np.random.default_rng(seed + s)
        x = rng.standard_normal(n) * 3000
        y = rng.standard_normal(n) * 3000
        if kind == "tones":
            p = H.gen_pcm(F, 2, seed=seed + s, kind="tones").astype(np.float64)
            l, r = p[:, 0], p[:, 1]
        elif kind == "noise":
            l, r = x, y
        elif kind == "identical":
            l = r = x + 4000 * np.sin(2 * np.pi * 1700.0 / 48000.0 * t)
        elif kind == "nearmono":
            l, r = x + 0.05 * y, x - 0.05 * y
        elif kind in ("music_identical", "music_nearmono"):      # tonal content (the harness's music), mono or near it
            p = H.gen_pcm(F, 2, seed=seed + s, kind="music").astype(np.float64)
            l = r = p[:, 0]
            if kind == "music_nearmono":
                l, r = p[:, 0] + 0.05 * p[:, 1], p[:, 0] - 0.05 * p[:, 1]
        elif kind == "changing":                # the correlation changes from block to block
            c = np.repeat(rng.uniform(-1.0, 1.0, n // 256 + 1), 256)[:n]
            l, r = x, c * x + np.sqrt(1 - c * c) * y
        elif kind == "quietR":                  # R 40 dB below L, independent
            l, r = x, 0.01 * y
        elif kind == "silentR":
            l, r = x, 0 * y
        elif kind == "attack":                  # a steady correlated bed, tone bursts in one channel or both: mixed blksw
            bed = 3000 * np.sin(2 * np.pi * 200.0 / 48000.0 * t) + 600 * np.sin(2 * np.pi * 2500.0 / 48000.0 * t)
            l = bed + rng.integers(-20, 21, n)
            r = bed + rng.integers(-20, 21, n)
            for f in range(F):
                o = 1536 * f + 256 * int(rng.integers(0, 6)) + int(rng.integers(0, 256))
                m = (t >= o) & (t < o + 400)
                burst = 16000 * np.sin(2 * np.pi * 3000.0 / 48000.0 * (t[m] - o))
                l[m] += burst
                if f % 2:
                    r[m] += burst
        else:
            raise ValueError(kind)
        out.append(np.stack([l, r], -1))
    return np.clip(np.round(np.array(out)), -32768, 32767).astype(np.int16)


def _expect(engine, pcm, bsw=0, lasts=None):
    """The model's mode-1 rows, shifts, flags and rematstr [S][F][6]... from the mode-0 taps of the same content."""
    import torch
    last0 = None if lasts is None else torch.from_numpy(np.ascontiguousarray(lasts)).cuda()
    _, t0 = _encode(engine, pcm, 2, 0, bsw=bsw, taps=True, last=last0)
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
    frames, t1 = _encode(engine, pcm, 2, 1, bsw=bsw, taps=True)
    assert np.array_equal(t1["mdct"], rows), np.argwhere(t1["mdct"] != rows)[:8]
    assert np.array_equal(t1["exp_samples"], shift)
    return frames, flags, rs


def _block0_bits(frames):
    """rematstr and the four flags of block 0: bits 74..78 of this encoder's 2/0 frames (67 bits of header; blksw x2,
    dithflag x2, dynrnge, cplstre, cplinu)."""
    bits = np.unpackbits(frames[..., :10], axis=-1)
    return bits[..., 74], (bits[..., 75] | bits[..., 76] << 1 | bits[..., 77] << 2 | bits[..., 78] << 3)


@pytest.mark.parametrize("nch", [1, 2, 6])
def test_off_and_non_stereo_are_the_reference(engine, nch):
    for kind in ("tones", "music"):
        pcm = np.stack([H.gen_pcm(2, nch, seed=31 + s, kind=kind) for s in range(2)])
        want = np.stack([H.orc_encode(p, nch, RATE[nch], chmap=(_chmap(nch) + (0,) * 8)[:8]) for p in pcm])
        assert np.array_equal(_encode(engine, pcm, nch, 0), want), kind
        if nch != 2:
            assert np.array_equal(_encode(engine, pcm, nch, 1), want), kind
        assert np.array_equal(_encode(engine, pcm, nch, 0), want), kind


@pytest.mark.parametrize("kind", ["quietR", "silentR"])
def test_no_qualifying_band_is_the_reference(engine, kind):
    pcm = _stereo(kind, 2, 3, seed=41)
    (_, _, flags, _), _ = _expect(engine, pcm)
    assert flags.sum() == 0
    want = np.stack([H.orc_encode(p, 2, RATE[2], chmap=(0, 1) + (0,) * 6) for p in pcm])
    assert np.array_equal(_encode(engine, pcm, 2, 1), want)


@pytest.mark.parametrize("pack", [1, 2])
@pytest.mark.parametrize("F", [1, 3])
def test_rows_equal_the_model(engine, pack, F):
    engine.set_encode_mode(pack)
    try:
        for kind in ("tones", "noise", "identical", "nearmono", "changing"):
            pcm = _stereo(kind, 3, F, seed=51)
            frames, flags, rs = _check_rows(engine, pcm)
            if kind in ("identical", "nearmono"):
                assert flags.min() == 15, kind
            if kind == "changing" and F == 3:
                assert 0 < flags.astype(bool).mean() < 1 and rs[:, :, 1:].sum() > 0
            got_rs, got_fl = _block0_bits(frames)
            assert np.array_equal(got_rs, np.ones_like(got_rs)) and np.array_equal(got_fl, flags[:, :, 0]), kind
    finally:
        engine.set_encode_mode(0)


@pytest.mark.parametrize("pack", [1, 2])
def test_rows_with_block_switching(engine, pack):
    engine.set_encode_mode(pack)
    try:
        pcm = _stereo("attack", 3, 3, seed=57)
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
    pcm = _stereo("changing", S, F, seed=61)
    whole, flags, _ = _check_rows(engine, pcm)
    assert flags.sum() > 0
    last = torch.zeros((S, 2, 256), dtype=torch.int16, device="cuda")
    csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
    a = _encode(engine, pcm[:, :2 * 1536], 2, 1, last=last, csnr=csnr)
    lasts = last.cpu().numpy()
    b, t = _encode(engine, pcm[:, 2 * 1536:], 2, 1, last=last, csnr=csnr, taps=True)
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
            got.append(_encode(engine, pcm[:, f * 1536:(f + 1) * 1536], 2, 1,
                               last=last6.view(-1)[:S * 2 * 256].view(S, 2, 256), csnr=csnr6))
    finally:
        engine._check(engine.lib.ac3mi_set_state_slots(ctypes.c_void_p(engine.ctx), None))
    assert np.array_equal(np.concatenate(got, 1), whole)


def _gpu_decode(engine, frames):
    import torch
    pkg = H.pkg()
    S, F, fb = frames.shape
    stride = (fb + 3) & ~3
    buf = np.zeros((S, F, stride), np.uint8)
    buf[:, :, :fb] = frames
    dec = pkg.DecodeDesc(flags=2, level=1.0, bias=0.0, dynrng=1, acmod=2, lfeon=0, frame_bytes=fb)
    delay = torch.zeros((S, 2, 128), dtype=torch.float32, device="cuda")
    lfsr = torch.ones((S,), dtype=torch.int16, device="cuda")
    out, status = engine.decode_batch(dec, torch.from_numpy(buf).cuda(), delay, lfsr)
    engine.sync()
    return out.cpu().numpy(), status.cpu().numpy()


def test_rematrixed_streams_decode_like_liba52(engine):
    import bench
    pcm = np.concatenate([_stereo(k, 1, 3, seed=71) for k in ("identical", "nearmono", "changing", "tones")])
    for bsw in (0, 1):
        frames = _encode(engine, pcm, 2, 1, bsw=bsw)
        assert bench.ac3_crc_ok(frames.reshape(-1, frames.shape[2])) == 0
        got, status = _gpu_decode(engine, frames)
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
        pcm = _stereo(kind, 1, F, seed=81)
        f0, t0 = _encode(engine, pcm, 2, 0, taps=True, rate=96000)
        f1, t1 = _encode(engine, pcm, 2, 1, taps=True, rate=96000)
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
    pools = {k: _stereo(k, 8, 1, seed=92) for k in kinds}
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
    src = _encode(engine, np.concatenate([_stereo(k, 1, F, seed=101) for k in ("nearmono", "changing", "tones")]), 2, 1)
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
    assert _block0_bits(out.cpu().numpy()[:, :, :fb])[1].sum() > 0


def test_setter_rejects_other_modes(engine):
    pcm = _stereo("nearmono", 1, 2, seed=111)
    on = _encode(engine, pcm, 2, 1)
    off = _encode(engine, pcm, 2, 0)
    assert not np.array_equal(on, off)
    engine.set_encode_rematrix(1)
    try:
        for m in (-1, 2):
            with pytest.raises(Exception):
                engine.set_encode_rematrix(m)
        assert np.array_equal(_encode(engine, pcm, 2, None), on)        # still mode 1
    finally:
        engine.set_encode_rematrix(0)
    assert np.array_equal(_encode(engine, pcm, 2, None), off)
