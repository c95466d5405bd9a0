"""GPU: cost-based exponent strategies in the encoder (ac3mi_set_encode_exp_strategy).  Mode 0 set explicitly is the
default byte for byte; mode 1's strategies and exponents follow the numpy model (tests/exp_strategy_model.py) on the raw
exponents of the mode-0 taps, for uncoupled channels, the LFE, coupled channels and the coupling channel; only the choice
changes; the streams decode cleanly; call shapes, transcode, a large batch, the setter and the other layers; and the
quality figures of DESIGN.md 4.3f."""
import ctypes

import numpy as np
import pytest

from tests import _harness as H
from tests import _tools as T
from tests import bandwidth_model as W
from tests import exp_strategy_model as X

pytestmark = pytest.mark.gpu


def _pcm(nch, S, F, seed, kinds=("music", "attack", "noise", "identical")):
    return np.concatenate([T.content(k, nch, 1, F, seed=seed + i) for i, k in enumerate(kinds)])[:S]


def test_setter_validates_and_keeps_the_setting(engine):
    for m in (-1, 2, 7):
        with pytest.raises(Exception):
            engine.set_encode_exp_strategy(m)
    pcm = _pcm(2, 2, 2, seed=5)
    on = T.encode(engine, pcm, xs=1)
    engine.set_encode_exp_strategy(1)
    try:
        with pytest.raises(Exception):
            engine.set_encode_exp_strategy(2)
        assert np.array_equal(T.encode(engine, pcm, xs=T.KEEP), on)        # the bad call left mode 1
    finally:
        engine.set_encode_exp_strategy(0)
    assert np.array_equal(T.encode(engine, pcm, xs=T.KEEP), T.encode(engine, pcm))


@pytest.mark.parametrize("nch", [1, 2, 6])
def test_off_means_unchanged(engine, nch):
    """Mode 0 set explicitly gives the bytes of never calling the setter, with every other tool off and on."""
    pcm = _pcm(nch, 3, 2, seed=11)
    combos = [dict(), dict(bsw=1), dict(bw=(1, 25))]
    if nch >= 2:
        combos.append(dict(cpl=(1, 2), bsw=1))
    if nch == 2:
        combos.append(dict(remat=1, cpl=(1, 3), bw=(1, 30)))
    for kw in combos:
        want = T.encode(engine, pcm, xs=T.KEEP, **kw)
        assert np.array_equal(T.encode(engine, pcm, xs=0, **kw), want), kw
        assert not np.array_equal(T.encode(engine, pcm, xs=1, **kw), want), kw


@pytest.mark.parametrize("nch", [1, 2, 6])
@pytest.mark.parametrize("sr", [48000, 44100, 32000])
def test_matches_the_model(engine, nch, sr):
    """Mode-1 d_exp_strategy and d_encoded_exp on [0, nbc) are the model's on the d_exponent tap, with block switching,
    rematrixing and bandwidth on and off."""
    pcm = _pcm(nch, 4, 2, seed=21)
    combos = [(dict(), 223), (dict(bsw=1), 223), (dict(bw=(1, 13)), W.nbc(13)), (dict(bw=(1, 40), bsw=1), W.nbc(40))]
    if nch == 2:
        combos += [(dict(remat=1), 223), (dict(remat=1, bsw=1, bw=(1, 25)), W.nbc(25))]
    for kw, n in combos:
        frames, t1 = T.encode(engine, pcm, xs=1, taps=True, sr=sr, **kw)
        T.check_rows(t1, nch, n)
        if sr == 48000:
            T.decodes_cleanly(frames, *T.layout_of(nch), engine=engine)


@pytest.mark.parametrize("nch,begf", [(2, 0), (2, 5), (6, 2)])
def test_coupled_frames_follow_the_model(engine, nch, begf):
    """In a coupled frame the coupled channels choose over [0, cplstrtmant) (gainrng, no chbwcod) and the coupling
    channel over [cplstrtmant, 217); its exponents are read back from the GPU decoder's coupling plane
    (tests/_tools.check_coupled_frames)."""
    pcm = np.concatenate([T.content("music", nch, 3, 2, seed=41), T.content("identical", nch, 1, 2, seed=45)])
    assert T.check_coupled_frames(engine, pcm, nch, begf) > 0


def test_only_the_choice_changes(engine):
    """Rows, raw exponents and exp_samples are mode 0's; J(mode 1) <= J(mode 0) on every channel-frame; the content reaches
    sequences mode 0 never sends: lone D15 sets, and D25 / D45 runs of four blocks or more (or D45 runs of two or more), the
    latter on quiet stationary streams (low-level noise, a soft tone) whose exponents are flat enough for coarse groups."""
    rng = np.random.default_rng(62)
    n = 3 * 1536
    quiet = np.stack([np.round(rng.standard_normal((n, 6)) * 3), np.round(
        np.sin(2 * np.pi * 1000.0 / 48000.0 * np.arange(n))[:, None] * np.full(6, 40.0))]).astype(np.int16)
    pcm = np.concatenate([_pcm(6, 4, 3, seed=61), quiet])
    for kw in (dict(), dict(bsw=1)):
        _, t0 = T.encode(engine, pcm, xs=0, taps=True, **kw)
        _, t1 = T.encode(engine, pcm, xs=1, taps=True, **kw)
        for k in ("mdct", "exponent", "exp_samples"):
            assert np.array_equal(t0[k], t1[k]), k
        seqs = T.check_rows(t1, 6, 223)
        S, F = pcm.shape[0], pcm.shape[1] // 1536
        for s in range(S):
            for f in range(F):
                for ch in range(6):
                    k, hi = ("lfe", 7) if ch == 5 else ("fbw", 223)
                    raw = t0["exponent"][s, f, :, ch].astype(np.int64)
                    j0 = X.seq_cost(k, raw, [int(v) for v in t0["exp_strategy"][s, f, :, ch]], 0, hi)
                    j1 = X.seq_cost(k, raw, [int(v) for v in t1["exp_strategy"][s, f, :, ch]], 0, hi)
                    assert j1 <= j0, (s, f, ch)
    lone15 = long_coarse = False
    for k, st in seqs:
        runs = []
        b = 0
        while b < 6:
            e = b + 1
            while e < 6 and st[e] == 0:
                e += 1
            runs.append((st[b], e - b))
            b = e
        lone15 |= any(s == 1 and L == 1 for s, L in runs)
        long_coarse |= any(s in (2, 3) and L >= 4 for s, L in runs) or any(s == 3 and L >= 2 for s, L in runs)
    print("lone D15 sets: %s, long D25 / D45 runs: %s" % (lone15, long_coarse))
    assert lone15 and long_coarse


def test_decodes_cleanly_and_exponents_round_trip(engine):
    """Mode-1 streams decode without errors through the liba52 restatement, the real liba52 where it was built, and the
    GPU decoder; the decoded exponents are d_encoded_exp."""
    for nch in (2, 6):
        pcm = _pcm(nch, 4, 2, seed=71)
        frames, t1 = T.encode(engine, pcm, xs=1, bsw=1, taps=True)
        T.decodes_cleanly(frames, *T.layout_of(nch), engine=engine)
        _, status, tp = T.decode(engine, frames, *T.layout_of(nch), taps=True)
        flags = T.ACMOD[nch] | (16 if nch == 6 else 0)
        for ch in range(nch):
            k = 7 if nch == 6 and ch == 5 else 223
            assert np.array_equal(t1["encoded_exp"][:, :, :, ch, :k], tp["exp"][:, :, :, ch, :k]), ch
        if H.have_ref():
            for s in range(frames.shape[0]):
                _, errs, _ = H.ref_decode(frames[s], flags, 1.0, 0.0)
                assert errs == 0


def test_call_shapes_and_packers_agree(engine):
    """One call, per-frame calls (history and csnr carried), state slots, a small tile, and both packer variants give the
    same bytes; transcode is decode + convert_s16 + encode byte for byte and state for state."""
    import torch
    pkg = H.pkg()
    S, F, nch = 3, 3, 6
    pcm = _pcm(nch, S, F, seed=81)
    for kw in (dict(), dict(cpl=(1, 1), bsw=1, bw=(1, 40))):
        want = T.encode(engine, pcm, xs=1, **kw)
        last = torch.zeros((S, nch, 256), dtype=torch.int16, device="cuda")
        csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
        per = [T.encode(engine, pcm[:, 1536 * f:1536 * (f + 1)], xs=1, last=last, csnr=csnr, **kw) for f in range(F)]
        assert np.array_equal(np.concatenate(per, 1), want), kw
        engine.set_tile_frames(2)
        try:
            assert np.array_equal(T.encode(engine, pcm, xs=1, **kw), want), kw
        finally:
            engine.set_tile_frames(0)
        for mode in (1, 2):
            engine.set_encode_mode(mode)
            try:
                assert np.array_equal(T.encode(engine, pcm, xs=1, **kw), want), (kw, mode)
            finally:
                engine.set_encode_mode(0)
    # transcode
    S, F = 4, 2
    src = np.stack([H.orc_encode(p, 2, 192000, chmap=(0, 1, 0, 0, 0, 0, 0, 0)) for p in _pcm(2, S, F, seed=85)])
    fb = src.shape[2]
    buf = np.zeros((S, F, (fb + 3) & ~3), np.uint8)
    buf[:, :, :fb] = src
    frames_t = torch.from_numpy(buf).cuda()
    dec = pkg.DecodeDesc(flags=2 | 32, level=1.0, bias=384.0, dynrng=1, acmod=2, lfeon=0, frame_bytes=fb)
    enc = pkg.EncodeDesc(48000, 192000, 2)
    engine.set_encode_exp_strategy(1)
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
        engine.set_encode_exp_strategy(0)
    assert int((status.cpu() & 0x1ff).max()) == 0
    assert torch.equal(out.cpu(), out2.cpu()) and torch.equal(last.cpu(), last2.cpu()) and torch.equal(csnr.cpu(), csnr2.cpu())
    T.decodes_cleanly(out.cpu().numpy()[:, :, :fb], 2, 0, engine=engine)


def test_large_batch(engine):
    """65 536 one-frame 5.1 streams in mode 1: both CRCs, clean decodes; a sample of them against the model."""
    import bench
    S = 65536
    rng = np.random.default_rng(91)
    pool = _pcm(6, 4, 1, seed=92)
    idx = rng.integers(0, len(pool), S)
    gain = rng.uniform(0.3, 1.0, (S, 1, 1))
    pcm = (pool[idx].astype(np.float64) * gain).astype(np.int16)
    frames = T.encode(engine, pcm, xs=1)
    assert bench.ac3_crc_ok(frames.reshape(-1, frames.shape[2])) == 0
    got, status, _ = T.decode(engine, frames, 7, 1)
    assert (status & 0x1ff).max() == 0
    pick = rng.integers(0, S, 16)
    _, t = T.encode(engine, pcm[pick], xs=1, taps=True)
    assert np.array_equal(T.encode(engine, pcm[pick], xs=1), frames[pick])
    T.check_rows(t, 6, 223)


def test_stream_layer_never_uses_it(engine):
    import importlib
    S = importlib.import_module("ac-3-acm-codec_amd.stream")
    pcm = H.gen_pcm(3, 6, seed=5, kind="music")
    want = H.orc_encode(pcm).tobytes()
    engine.set_encode_exp_strategy(1)
    pool = S.Pool(engine, 4)
    try:
        rc, st = pool.open(S.pcm_format(6, 48000), S.ac3_format(6, 48000, 384))
        assert rc == 0
        src = np.frombuffer(pcm.tobytes(), np.uint8).copy()
        dst = np.zeros(len(want) + 4096, np.uint8)
        h = S.StreamHeader(src.ctypes.data, src.size, 0, dst.ctypes.data, dst.size, 0, S.STREAMCONVERTF_START)
        assert st.convert(h) == 0
        st.close()
        assert bytes(dst[:h.dst_used]) == want[:h.dst_used] and h.dst_used > 0
        # the setting is still there for the batch calls
        assert not np.array_equal(T.encode(engine, np.asarray(pcm)[None], xs=T.KEEP), T.encode(engine, np.asarray(pcm)[None]))
    finally:
        pool.close()
        engine.set_encode_exp_strategy(0)


def _quality(engine, pcm, nch, rate, **kw):
    nfbw = min(nch, 5)
    o = 1 if nch == 6 else 0
    res = []
    for xs in (0, 1):
        fr, t = T.encode(engine, pcm, xs=xs, taps=True, rate=rate, **kw)
        T.decodes_cleanly(fr, *T.layout_of(nch), engine=engine)
        off = (16 * t["snroffst"][..., 0] + t["snroffst"][..., 1]).astype(np.float64).mean()
        x = t["mdct"].astype(np.float64) * np.exp2(-(23.0 + t["exp_samples"]))[..., None]
        x = x[:, :, :, :nfbw, :223]
        coef = T.decode(engine, fr, *T.layout_of(nch), taps=True)[2]["coef"].astype(np.float64)[:, :, :, o:o + nfbw, :223]
        res.append((off, 10 * np.log10((x ** 2).sum() / ((coef - x) ** 2).sum())))
    return res


# Measured on the MI355X when written, mean 16 csnroffst + fsnroffst and coefficient SNR, mode 0 -> mode 1:
#   2/0  96 kb/s  224.75 -> 233.25 (+8.50),  30.22 -> 29.80 dB (-0.43)
#   2/0 192 kb/s  289.62 -> 294.25 (+4.62),  41.52 -> 40.36 dB (-1.16)
#   5.1 224 kb/s  204.25 -> 205.50 (+1.25),  25.18 -> 24.48 dB (-0.71)
#   5.1 384 kb/s  258.25 -> 262.00 (+3.75),  36.18 -> 36.02 dB (-0.16)
#   re-encoded 2/0 192 kb/s  270.50 -> 273.38 (+2.88),  38.66 -> 40.09 dB (+1.44)
# The SNR offsets rise everywhere (the chosen sets cost fewer bits), but on music the coefficient SNR falls: at one bit per
# exponent step the model trades exponent precision for mantissa bits at a rate this content does not repay.  Only the
# re-encoded content gains in SNR, by 1.44 dB; its test asserts half of each gain, the others print their figures and
# assert only half of the smallest offset gain.
@pytest.mark.parametrize("nch,rate", [(2, 96000), (2, 192000), (6, 224000), (6, 384000)])
def test_quality_on_music(engine, nch, rate):
    """Mean 16 csnroffst + fsnroffst and the decoded coefficients' SNR against d_mdct, mode 0 against mode 1, on the
    harness's music (figures above).  Mode 1 raises the mean SNR offset (asserted: half of the smallest measured gain,
    +1.25) and loses 0.2 - 1.2 dB of coefficient SNR (printed, not asserted)."""
    pcm = T.content("music", nch, 2, 4, seed=53)
    (o0, s0), (o1, s1) = _quality(engine, pcm, nch, rate)
    print("%d ch %d kb/s: 16 csnr + fsnr %.2f -> %.2f (%+.2f); coefficient SNR %.2f -> %.2f dB (%+.2f)"
          % (nch, rate // 1000, o0, o1, o1 - o0, s0, s1, s1 - s0))
    assert o1 - o0 >= 0.6


def test_quality_on_reencoded_audio(engine):
    """The transcode's input: decoded AC-3 re-encoded (2/0, 192 kb/s).  Measured +2.88 in the mean SNR offset and +1.44 dB
    coefficient SNR; the thresholds keep about half of each."""
    S, F = 2, 4
    pcm = T.content("music", 2, S, F, seed=57)
    src = np.stack([H.orc_encode(p, 2, 192000, chmap=(0, 1, 0, 0, 0, 0, 0, 0)) for p in pcm])
    dec = np.stack([np.clip(np.round(H.orc_decode(src[s], 2, 1.0, 0.0)[0].transpose(0, 1, 3, 2).reshape(-1, 2) * 32768.0),
                            -32768, 32767) for s in range(S)]).astype(np.int16)
    (o0, s0), (o1, s1) = _quality(engine, dec, 2, 192000)
    print("re-encoded 2/0 192 kb/s: 16 csnr + fsnr %.2f -> %.2f (%+.2f); coefficient SNR %.2f -> %.2f dB (%+.2f)"
          % (o0, o1, o1 - o0, s0, s1, s1 - s0))
    assert o1 - o0 >= 1.4 and s1 - s0 >= 0.7


def test_pre_echo_with_block_switching(engine):
    """test_pre_echo's measurement (tests/test_block_switch_gpu.py: six attacks, error energy over the 256 samples before
    each onset, decoded with the liba52 restatement) with block switching on, mode 0 against mode 1.  Measured when
    written: mode 1 has 3.76 dB MORE pre-echo energy (6.83e8 -> 1.62e9).  The cost model prices exponent steps summed over
    the row and the run; it does not see where in time the error falls.  Printed, not asserted as a gain;
    both streams decode cleanly."""
    from tests import block_switch_model as M
    nch, F = 2, 8
    onsets = [1536 * f + 256 * (f % 6) + off for f, off in zip(range(1, F - 1), (20, 64, 100, 150, 200, 250))]
    pcm = M.attack_pcm(F, nch, onsets, amp=20000.0, seed=91)[None]
    e = {}
    for xs in (0, 1):
        frames = T.encode(engine, pcm, xs=xs, bsw=1)[0]
        out, errs, _ = H.orc_decode(frames, 2, 1.0, 0.0)
        assert errs == 0
        dec = out.transpose(0, 1, 3, 2).reshape(-1, nch).astype(np.float64) * 32768.0
        err = dec[256:] - pcm[0][:dec.shape[0] - 256].astype(np.float64)
        e[xs] = sum(float((err[o - 256:o] ** 2).sum()) for o in onsets)
    gain = 10 * np.log10(e[0] / e[1])
    print("pre-echo energy before %d onsets, block switching on: mode 0 %.4g, mode 1 %.4g: %.2f dB lower"
          % (len(onsets), e[0], e[1], gain))
    assert e[0] > 0 and e[1] > 0
