"""GPU: audio bandwidth in the encoder (ac3mi_set_encode_bandwidth).  Mode 1 at chbwcod 50 is mode 0 byte for byte with
every other coding tool; band-limited streams decode cleanly with the liba52 restatement and the GPU decoder, carry the
chosen chbwcod, decode to zero above nbc, keep mode 0's strategies, raw exponents and rows, and send the exponents and
baps of the numpy model (tests/bandwidth_model.py); mode 2 follows the model's table; rematrixing and coupling end where
the bandwidth says; call shapes, transcode, a large batch, the setter and the stream layer; and the quality gain."""
import ctypes

import numpy as np
import pytest

from tests import _harness as H
from tests import _tools as T
from tests import bandwidth_model as W
from tests import rematrix_model as M

pytestmark = pytest.mark.gpu


# encoder bap (0..15) -> liba52's convention (the GPU decoder's tap): grouped codes negative, plain widths in bits
_BAP52 = np.array([0, -1, -2, 3, -3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16], np.int8)


def _check_band_limited(engine, pcm, nch, c, frames, t1, t0):
    n, nfbw = W.nbc(c), min(nch, 5)
    S, F = frames.shape[:2]
    T.decodes_cleanly(frames, *T.layout_of(nch), engine=engine)
    for s in range(S):
        for f in range(F):
            assert T.uncoupled_view(frames[s, f], nch)[1] == [c] * nfbw, (s, f)
    _, status, tp = T.decode(engine, frames, *T.layout_of(nch), taps=True)
    assert (status & 0x1ff).max() == 0
    o = 1 if nch == 6 else 0                    # (the decoder's planes put the LFE first)
    assert not tp["coef"][:, :, :, o:o + nfbw, n:].any()
    # what does not depend on the bandwidth
    assert np.array_equal(t1["exp_strategy"], t0["exp_strategy"])
    assert np.array_equal(t1["exponent"], t0["exponent"])
    assert np.array_equal(t1["exp_samples"], t0["exp_samples"])
    assert np.array_equal(t1["mdct"][..., :n], t0["mdct"][..., :n])
    # the exponents sent: the model on mode 0's raw exponents and strategies; the LFE's are mode 0's
    for s in range(S):
        for f in range(F):
            for ch in range(nfbw):
                want = W.encode_exp(t0["exponent"][s, f, :, ch], t0["exp_strategy"][s, f, :, ch], n)
                assert np.array_equal(t1["encoded_exp"][s, f, :, ch, :n], want), (s, f, ch)
    if nch == 6:
        assert np.array_equal(t1["encoded_exp"][:, :, :, 5, :7], t0["encoded_exp"][:, :, :, 5, :7])
    # the encoder's bap is the one the decoder derives from the frames
    for ch in range(nch):
        k = 7 if nch == 6 and ch == 5 else n
        assert np.array_equal(_BAP52[t1["bap"][:, :, :, ch, :k]], tp["bap"][:, :, :, ch, :k]), ch
        assert np.array_equal(t1["encoded_exp"][:, :, :, ch, :k], tp["exp"][:, :, :, ch, :k]), ch


@pytest.mark.parametrize("nch", [1, 2, 6])
def test_chbwcod_50_is_mode0(engine, nch):
    """Mode 1 at chbwcod 50 runs the runtime-bandwidth kernels and gives mode 0's bytes with every tool."""
    combos = [dict(), dict(bsw=1)]
    if nch == 2:
        combos.append(dict(remat=1))
        combos.append(dict(remat=1, cpl=(1, 2)))
    if nch >= 2:
        combos += [dict(cpl=(1, 0)), dict(cpl=(1, 2)), dict(cpl=(1, 2), bsw=1)]
    for kw in combos:
        for kind in ("music", "attack"):
            pcm = T.content(kind, nch, 2, 3, seed=11)
            f0 = T.encode(engine, pcm, bw=(0, 50), **kw)
            f1 = T.encode(engine, pcm, bw=(1, 50), **kw)
            assert np.array_equal(f1, f0), (kw, kind)
    pcm = T.content("music", nch, 2, 3, seed=11)
    assert np.array_equal(T.encode(engine, pcm, bw=(0, 50)),
                          np.stack([H.orc_encode(p, nch, T.RATE[nch], chmap=(T.chmap_of(nch) + (0,) * 8)[:8]) for p in pcm]))


@pytest.mark.parametrize("nch", [1, 2, 6])
@pytest.mark.parametrize("c", [0, 13, 32, 49])
def test_band_limited_streams(engine, nch, c):
    for F in (1, 4):
        pcm = T.content("music", nch, 2, F, seed=17 + c)
        _, t0 = T.encode(engine, pcm, taps=True)
        for pack in (1, 2):
            engine.set_encode_mode(pack)
            try:
                frames, t1 = T.encode(engine, pcm, bw=(1, c), taps=True)
                plain = T.encode(engine, pcm, bw=(1, c))
            finally:
                engine.set_encode_mode(0)
            assert np.array_equal(plain, frames)            # (taps do not change the bytes)
            _check_band_limited(engine, pcm, nch, c, frames, t1, t0)


@pytest.mark.parametrize("nch,rate,sr", [(1, 64000, 48000), (2, 96000, 48000), (2, 192000, 48000), (2, 96000, 44100),
                                         (2, 64000, 32000), (6, 224000, 48000), (6, 384000, 48000), (6, 448000, 44100),
                                         (2, 48000, 24000)])
def test_mode2_follows_the_table(engine, nch, rate, sr):
    pcm = T.content("music", nch, 1, 2, seed=23)
    c = W.mode2_chbwcod(sr, rate, nch)
    frames = T.encode(engine, pcm, bw=(2, 7), rate=rate, sr=sr)
    for f in range(frames.shape[1]):
        assert T.uncoupled_view(frames[0, f], nch)[1] == [c] * min(nch, 5)
    assert np.array_equal(frames, T.encode(engine, pcm, bw=(1, c), rate=rate, sr=sr))


@pytest.mark.parametrize("c", [13, 32])
def test_rematrixing_band_ends_at_nbc(engine, c):
    """Coded rows and block-0 flags of 2/0 with rematrixing: the model with the fourth band [61, nbc)."""
    S, F, n = 2, 3, W.nbc(c)
    pcm = T.content("identical", 2, 1, F, seed=29)
    pcm = np.concatenate([pcm, T.content("music", 2, 1, F, seed=31)])
    _, t0 = T.encode(engine, pcm, taps=True)
    frames, t1 = T.encode(engine, pcm, bw=(1, c), remat=1, taps=True)
    T.decodes_cleanly(frames, 2, 0, engine=engine)
    n_on = 0
    for s in range(S):
        v = M.block_v(pcm[s], (0, 1))
        for f in range(F):
            for b in range(6):
                vl, vr = int(v[f, b, 0]), int(v[f, b, 1])
                rows = t0["mdct"][s, f, b].astype(np.int64)
                fl = W.remat_flags(rows[0], rows[1], vl - 9, vr - 9, n)
                n_on += fl != 0
                if b == 0:
                    assert T.uncoupled_view(frames[s, f], 2)[0] == fl, (s, f)
                if not fl:
                    assert np.array_equal(t1["mdct"][s, f, b, :, :n], t0["mdct"][s, f, b, :, :n])
                    continue
                vm = min(vl, vr)
                a, r = rows[0] >> (vl - vm), rows[1] >> (vr - vm)
                want = np.stack([a, r])
                for i, (lo, hi) in enumerate(W.remat_bands(n)):
                    if (fl >> i) & 1:
                        want[0, lo:hi] = (a[lo:hi] + r[lo:hi]) >> 1
                        want[1, lo:hi] = (a[lo:hi] - r[lo:hi]) >> 1
                sh = vm - 9
                if sh > 0:
                    want = np.where(np.abs(want) < (1 << sh), 0, want)
                assert np.array_equal(t1["mdct"][s, f, b, :, :n], want[:, :n]), (s, f, b)
                assert (t1["exp_samples"][s, f, b] == sh).all()
    assert n_on > 0


@pytest.mark.parametrize("nch", [2, 6])
def test_coupling_ends_at_cplendmant(engine, nch):
    """begf 2, chbwcod 32: coupled frames carry cplendf 8 and the model's side information, decode cleanly and have no
    coefficient from bin 169 on; begf 11 is beyond cplendf + 2: the bytes of coupling off at the same bandwidth."""
    begf, c, S, F = 2, 32, 2, 3
    nfbw = min(nch, 5)
    pcm = T.content("music", nch, S, F, seed=37)
    _, t0 = T.encode(engine, pcm, taps=True)
    frames = T.encode(engine, pcm, bw=(1, c), cpl=(1, begf))
    T.decodes_cleanly(frames, *T.layout_of(nch), engine=engine)
    n_on = 0
    for s in range(S):
        for f in range(F):
            want = W.cpl_decide(t0["mdct"][s, f], t0["exp_samples"][s, f], nfbw, begf, c)
            cplinu, chincpl, bf, ef, co = T.coupling_view(frames[s, f], nch)
            assert cplinu == want[0], (s, f)
            if cplinu:
                n_on += 1
                assert chincpl == (1 << nfbw) - 1 and bf == begf and ef == W.cplendf(c) == 8
                assert [m for m, _ in co] == want[1] and [cd for _, cd in co] == want[2], (s, f)
            else:
                assert T.uncoupled_view(frames[s, f], nch)[1] == [c] * nfbw
    assert n_on > 0
    _, status, tp = T.decode(engine, frames, *T.layout_of(nch), taps=True)
    o = 1 if nch == 6 else 0
    assert (status & 0x1ff).max() == 0 and not tp["coef"][:, :, :, o:o + nfbw, W.cplendmant(c):].any()
    assert np.array_equal(T.encode(engine, pcm, bw=(1, c), cpl=(1, 11)), T.encode(engine, pcm, bw=(1, c)))


def test_call_shapes_agree(engine):
    """Two calls of two frames, state slots, small tiles and both packers give the bytes of one call (5.1 band-limited;
    2/0 band-limited with coupling and rematrixing)."""
    import torch
    S, F = 3, 4
    perm = torch.tensor([2, 0, 1], dtype=torch.int32, device="cuda")
    for nch, kw in ((6, dict(bw=(1, 32))), (2, dict(bw=(1, 13), cpl=(1, 1), remat=1)), (6, dict(bw=(2, 0), rate=224000))):
        pcm = T.content("music", nch, S, F, seed=41)
        whole = T.encode(engine, pcm, **kw)
        for pack in (1, 2):
            engine.set_encode_mode(pack)
            try:
                assert np.array_equal(T.encode(engine, pcm, **kw), whole), (nch, pack)
            finally:
                engine.set_encode_mode(0)
        last = torch.zeros((S, nch, 256), dtype=torch.int16, device="cuda")
        csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
        a = T.encode(engine, pcm[:, :2 * 1536], last=last, csnr=csnr, **kw)
        b = T.encode(engine, pcm[:, 2 * 1536:], last=last, csnr=csnr, **kw)
        assert np.array_equal(np.concatenate([a, b], 1), whole), nch
        last6 = torch.zeros((S, 6, 256), dtype=torch.int16, device="cuda")
        csnr6 = torch.full((S,), 40, dtype=torch.int32, device="cuda")
        engine._check(engine.lib.ac3mi_set_state_slots(ctypes.c_void_p(engine.ctx), ctypes.c_void_p(perm.data_ptr())))
        try:
            got = [T.encode(engine, pcm[:, f * 1536:(f + 1) * 1536], last=last6.view(-1)[:S * nch * 256].view(S, nch, 256),
                           csnr=csnr6, **kw) for f in range(F)]
        finally:
            engine._check(engine.lib.ac3mi_set_state_slots(ctypes.c_void_p(engine.ctx), None))
        assert np.array_equal(np.concatenate(got, 1), whole), nch
        engine._check(engine.lib.ac3mi_set_tile_frames(ctypes.c_void_p(engine.ctx), ctypes.c_longlong(4)))
        try:
            tiled = T.encode(engine, pcm, **kw)
        finally:
            engine._check(engine.lib.ac3mi_set_tile_frames(ctypes.c_void_p(engine.ctx), ctypes.c_longlong(0)))
        assert np.array_equal(tiled, whole), nch


def test_transcode_equals_decode_then_encode(engine):
    import torch
    pkg = H.pkg()
    S, F, nch = 3, 3, 2
    src = T.encode(engine, T.content("music", nch, S, F, seed=101))
    fb = src.shape[2]
    stride = (fb + 3) & ~3
    buf = np.zeros((S, F, stride), np.uint8)
    buf[:, :, :fb] = src
    frames_t = torch.from_numpy(buf).cuda()
    dec = pkg.DecodeDesc(flags=2 | 32, level=1.0, bias=384.0, dynrng=1, acmod=2, lfeon=0, frame_bytes=fb)
    enc = pkg.EncodeDesc(48000, 96000, 2)
    engine.set_encode_bandwidth(2)
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
        engine.set_encode_bandwidth(0)
        engine.set_encode_coupling(0, 0)
    assert int((status.cpu() & 0x1ff).max()) == 0
    assert torch.equal(out.cpu(), out2.cpu()) and torch.equal(last.cpu(), last2.cpu()) and torch.equal(csnr.cpu(), csnr2.cpu())
    o = out.cpu().numpy()[:, :, :fb]
    T.decodes_cleanly(o, 2, 0, engine=engine)
    # (music at 96 kb/s: chbwcod 25 from the table, cplendf 6 in coupled frames)
    assert any(T.coupling_view(o[s, f], 2)[3] == 6 for s in range(S) for f in range(F))


def test_large_batch(engine):
    """4 096 one-frame 5.1 streams, band-limited with coupling: both CRCs, clean decodes, no coefficient above nbc."""
    import bench
    S, c = 4096, 13
    rng = np.random.default_rng(91)
    pool = np.concatenate([T.content(k, 6, 4, 1, seed=92) for k in ("music", "identical", "noise")])
    pcm = np.stack([pool[rng.integers(0, len(pool))] for _ in range(S)])
    pcm = (pcm.astype(np.int32) * rng.uniform(0.3, 1.0, (S, 1, 1))).astype(np.int16)
    for kw in (dict(), dict(cpl=(1, 0))):
        frames = T.encode(engine, pcm, bw=(1, c), **kw)
        assert bench.ac3_crc_ok(frames.reshape(-1, frames.shape[2])) == 0
        got, status, _ = T.decode(engine, frames, 7, 1)
        assert (status & 0x1ff).max() == 0
        ref, errs, _ = H.orc_decode(frames[:64, 0], 7 | 16, 1.0, 0.0)
        assert errs == 0
        _, _, tp = T.decode(engine, frames[:256], 7, 1, taps=True)
        assert not tp["coef"][:, :, :, 1:6, W.nbc(c):].any()


def test_coupled_exponent_tap_is_reproducible(engine):
    """Without the d_mdct tap the rows are stored below nbc only; a coupled channel's exponents above that are not read from
    whatever an earlier call left in the workspace: the d_encoded_exp / d_bap taps of a band-limited coupled call are the
    same after different earlier calls."""
    import torch
    pkg = H.pkg()
    S, F, nch, c = 4, 2, 6, 13
    pcm = T.content("music", nch, S, F, seed=59)
    enc = pkg.EncodeDesc(48000, 384000, nch)
    cm = (ctypes.c_uint8 * 8)(*(list(T.chmap_of(nch)) + [0] * 8)[:8])
    got = []
    for k, other in enumerate(("noise", "identical")):
        T.encode(engine, T.content(other, nch, S, F, seed=61 + k))          # (fills the workspace rows up to bin 223)
        t = {n: torch.full((S, F, 6, nch, 256), 0x5a, dtype=torch.uint8, device="cuda") for n in ("eexp", "bap")}
        tp = H.pkg().capi.EncodeTapsC(None, None, None, t["eexp"].data_ptr(), t["bap"].data_ptr(), None, None)
        last = torch.zeros((S, nch, 256), dtype=torch.int16, device="cuda")
        csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
        x = torch.from_numpy(np.ascontiguousarray(pcm).reshape(S, F, 1536, nch)).cuda()
        out = torch.zeros((S, F, (enc.frame_bytes() + 3) & ~3), dtype=torch.uint8, device="cuda")
        engine.set_encode_bandwidth(1, c)
        engine.set_encode_coupling(1, 0)
        try:
            dc = enc.c()
            engine._check(engine.lib.ac3mi_encode_batch(engine.ctx, ctypes.byref(dc), x.data_ptr(), cm, last.data_ptr(),
                                                        csnr.data_ptr(), out.data_ptr(), out.shape[2], S, F, ctypes.byref(tp)))
            engine.sync()
        finally:
            engine.set_encode_bandwidth(0)
            engine.set_encode_coupling(0, 0)
        got.append((out.cpu().numpy(), t["eexp"].cpu().numpy(), t["bap"].cpu().numpy()))
    assert any(T.coupling_view(got[0][0][s, f, :out.shape[2]], nch)[0] for s in range(S) for f in range(F))
    for a, b in zip(got[0], got[1]):
        assert np.array_equal(a, b)


def test_transcode_rejects_a_bad_encode_descriptor_in_mode2(engine):
    """Mode 2 reads the encode descriptor's channels and bit rate; a descriptor the encoder rejects (0 or 7 channels, a
    bit rate that is no AC-3 rate) gives AC3MI_ERR_ARG before anything uses it.  In a child process, so that a host fault
    there fails this test instead of ending the session."""
    import subprocess
    import sys
    code = """
import ctypes, sys, torch
sys.path.insert(0, %r)
from tests import _harness as H
pkg = H.pkg()
eng = pkg.Engine(0)
eng.set_encode_bandwidth(2)
S, F, fb = 1, 1, 768
frames = torch.zeros((S, F, fb), dtype=torch.uint8, device="cuda")
dec = pkg.DecodeDesc(flags=2 | 32, level=1.0, bias=384.0, dynrng=1, acmod=2, lfeon=0, frame_bytes=fb).c()
delay = torch.zeros((S, 6, 128), dtype=torch.float32, device="cuda")
lfsr = torch.ones((S,), dtype=torch.int16, device="cuda")
last = torch.zeros((S, 6, 256), dtype=torch.int16, device="cuda")
csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
out = torch.zeros((S, F, 4096), dtype=torch.uint8, device="cuda")
status = torch.zeros((S, F), dtype=torch.int32, device="cuda")
cm = (ctypes.c_uint8 * 8)(0, 1, 2, 3, 4, 5, 0, 0)
rcs = []
for ch, rate in ((0, 192000), (7, 192000), (2, 191000)):
    enc = pkg.EncodeDesc(48000, rate, ch).c()
    rcs.append(eng.lib.ac3mi_transcode_batch(eng.ctx, ctypes.byref(dec), ctypes.byref(enc), frames.data_ptr(), fb, S, F,
                                             delay.data_ptr(), lfsr.data_ptr(), cm, last.data_ptr(), csnr.data_ptr(),
                                             out.data_ptr(), 4096, status.data_ptr()))
eng.set_encode_bandwidth(0)
eng.close()
print("RCS", rcs)
""" % H.ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("RCS")] == ["RCS [-1, -1, -1]"], r.stdout[-2000:]


def test_setter_rejects_bad_arguments(engine):
    for mode, c in ((-1, 50), (3, 50), (1, -1), (1, 51), (1, 60)):
        with pytest.raises(Exception):
            engine.set_encode_bandwidth(mode, c)
    pcm = T.content("music", 2, 1, 2, seed=47)
    on = T.encode(engine, pcm, bw=(1, 13))
    engine.set_encode_bandwidth(1, 13)
    try:
        with pytest.raises(Exception):
            engine.set_encode_bandwidth(1, 51)
        assert np.array_equal(T.encode(engine, pcm, bw=T.KEEP), on)     # the bad call left mode 1, chbwcod 13
        engine.set_encode_bandwidth(2, 99)                              # (mode 2 and 0 ignore the argument)
        engine.set_encode_bandwidth(0, -5)
    finally:
        engine.set_encode_bandwidth(0)
    assert np.array_equal(T.encode(engine, pcm, bw=T.KEEP), T.encode(engine, pcm))


def test_stream_layer_never_band_limits(engine):
    import importlib
    S = importlib.import_module("ac-3-acm-codec_amd.stream")
    pcm = H.gen_pcm(3, 6, seed=5, kind="music")
    want = H.orc_encode(pcm).tobytes()
    engine.set_encode_bandwidth(1, 0)
    engine.set_encode_coupling(1, 0)
    engine.set_encode_rematrix(1)
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
        # the bandwidth setting is still there for the batch calls (coupling off for this one, so that every frame is
        # an uncoupled one that sends chbwcod)
        b = T.encode(engine, np.asarray(pcm)[None], bw=T.KEEP, cpl=(0, 0))
        assert not any(T.coupling_view(b[0, f], 6)[0] for f in range(b.shape[1]))
        assert all(T.uncoupled_view(b[0, f], 6)[1] == [0] * 5 for f in range(b.shape[1]))
    finally:
        pool.close()
        engine.set_encode_bandwidth(0)
        engine.set_encode_coupling(0, 0)
        engine.set_encode_rematrix(0)


@pytest.mark.parametrize("nch,rate,min_off,min_snr", [(2, 96000, 7.0, 0.9), (6, 224000, 14.0, 3.5)])
def test_quality_mode2_against_mode0(engine, nch, rate, min_off, min_snr):
    """On the harness's music the band-limited encode spends its bits below nbc: mean 16 csnroffst + fsnroffst rises, and
    so does the decoded coefficients' SNR on [0, nbc) against d_mdct.  Measured when written: 2/0 at
    96 kb/s (chbwcod 25) +14.3 and 32.80 -> 34.63 dB; 5.1 at 224 kb/s (chbwcod 14) +28.5 and 26.05 -> 33.04 dB.  The
    thresholds keep about half of each gain."""
    F = 6
    nfbw = min(nch, 5)
    pcm = T.content("music", nch, 1, F, seed=53)
    c = W.mode2_chbwcod(48000, rate, nch)
    n = W.nbc(c)
    f0, t0 = T.encode(engine, pcm, taps=True, rate=rate)
    f2, t2 = T.encode(engine, pcm, bw=(2, 0), taps=True, rate=rate)
    T.decodes_cleanly(f2, *T.layout_of(nch), engine=engine)
    o0 = (16 * t0["snroffst"][0, :, 0] + t0["snroffst"][0, :, 1]).astype(np.float64)
    o2 = (16 * t2["snroffst"][0, :, 0] + t2["snroffst"][0, :, 1]).astype(np.float64)
    x = t0["mdct"][0].astype(np.float64) * np.exp2(-(23.0 + t0["exp_samples"][0]))[..., None]
    x = x[:, :, :nfbw, :n]
    o = 1 if nch == 6 else 0
    snr = []
    for fr in (f0, f2):
        coef = T.decode(engine, fr, *T.layout_of(nch), taps=True)[2]["coef"][0].astype(np.float64)[:, :, o:o + nfbw, :n]
        snr.append(10 * np.log10((x ** 2).sum() / ((coef - x) ** 2).sum()))
    print("%d ch %d kb/s: chbwcod %d (nbc %d); 16 csnr + fsnr %s -> %s (mean %+.1f); coefficient SNR on [0, nbc) "
          "%.2f -> %.2f dB (%+.2f)" % (nch, rate // 1000, c, n, o0.tolist(), o2.tolist(), (o2 - o0).mean(), snr[0], snr[1],
                                       snr[1] - snr[0]))
    assert t0["snroffst"][0, :, 0].max() < 63
    assert (o2 - o0).mean() >= min_off, (o0, o2)
    assert snr[1] - snr[0] >= min_snr, snr
