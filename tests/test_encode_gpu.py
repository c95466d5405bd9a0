"""GPU parity: ac3mi_encode_batch (HIP) vs the ac3enc restatement in oracle/.

Reference behaviour under test: AC3_encode_frame (src/ac3enc/ac3enc.cpp:1640-1763).  Integer work:
every stage and the final bitstream must be BIT-EXACT against the oracle.  (The oracle itself is pinned
byte for byte to ac3enc by tests/test_oracle_vs_ac3enc.py; tests/test_encode_ref_gpu.py holds the engine
against frames recorded from ac3enc directly - see DESIGN.md §3.)
"""
import ctypes

import numpy as np
import pytest

from tests import _harness as H
from tests import variant_matrix as V

pytestmark = pytest.mark.gpu


def _oracle(pcm_streams, nch, bitrate, freq=48000, chmap=H.CHMAP6):
    """pcm_streams [S][F*1536][nch] -> frames [S][F][fb] + stage taps"""
    L = H.orc()
    S = len(pcm_streams)
    F = pcm_streams[0].shape[0] // 1536
    fb = H.ci()
    cm = (ctypes.c_uint8 * 8)(*chmap)
    frames = None
    taps = {k: [] for k in ("mdct", "exponent", "encoded_exp", "bap", "strat", "shift", "snr")}
    for s in range(S):
        h = L.orc_ac3enc_init(freq, bitrate, nch, ctypes.byref(fb))
        assert h
        if frames is None:
            frames = np.zeros((S, F, fb.value), np.uint8)
        pcm = np.ascontiguousarray(pcm_streams[s])
        for f in range(F):
            r = L.orc_ac3enc_frame(h, H.P(frames[s, f], H.u8p), ctypes.cast(pcm.ctypes.data + f * 1536 * nch * 2, H.i16p), cm)
            assert r == fb.value
            m = np.zeros((6, 6, 256), np.int32)
            e1, e2 = np.zeros((6, 6, 256), np.uint8), np.zeros((6, 6, 256), np.uint8)
            b = np.zeros((6, 6, 256), np.uint8)
            st, sh = np.zeros((6, 6), np.uint8), np.zeros((6, 6), np.int8)
            c, fs = H.ci(), H.ci()
            L.orc_ac3enc_get_mdct(h, H.P(m, H.i32p))
            L.orc_ac3enc_get_exp(h, H.P(e1, H.u8p), H.P(e2, H.u8p))
            L.orc_ac3enc_get_bap(h, H.P(b, H.u8p))
            L.orc_ac3enc_get_misc(h, H.P(st, H.u8p), H.P(sh, H.i8p), ctypes.byref(c), ctypes.byref(fs))
            for k, v in (("mdct", m), ("exponent", e1), ("encoded_exp", e2), ("bap", b), ("strat", st), ("shift", sh),
                         ("snr", np.array([c.value, fs.value]))):
                taps[k].append(v)
        L.orc_ac3enc_free(h)
    for k in taps:
        taps[k] = np.array(taps[k]).reshape((S, F) + np.array(taps[k][0]).shape)
    return frames, taps


def _gpu(engine, pcm_streams, nch, bitrate, freq=48000, chmap=H.CHMAP6, taps=True, split=None):
    import torch
    pkg = H.pkg()
    desc = pkg.EncodeDesc(freq, bitrate, nch)
    fb = desc.frame_bytes()
    S = len(pcm_streams)
    F = pcm_streams[0].shape[0] // 1536
    pcm = torch.from_numpy(np.stack(pcm_streams).reshape(S, F, 1536, nch)).cuda()
    last = torch.zeros((S, nch, 256), dtype=torch.int16, device="cuda")
    csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
    if split is None:
        res = engine.encode_batch(desc, pcm, chmap[:nch], last, csnr, taps=taps)
        engine.sync()
        out = res[0] if taps else res
        t = {k: v.cpu().numpy() for k, v in res[1].items()} if taps else None
        return out.cpu().numpy()[:, :, :fb], t
    a = engine.encode_batch(desc, pcm[:, :split].contiguous(), chmap[:nch], last, csnr)
    b = engine.encode_batch(desc, pcm[:, split:].contiguous(), chmap[:nch], last, csnr)
    engine.sync()
    return np.concatenate([a.cpu().numpy(), b.cpu().numpy()], axis=1)[:, :, :fb], None


@pytest.mark.parametrize("kind", ["tones", "noise", "quiet", "music", "bursts", "strobe"])
def test_encode_5_1_all_stages(engine, kind):
    S, F = 5, 3
    pcm = [H.gen_pcm(F, 6, seed=31 + 7 * s, kind=kind) for s in range(S)]
    want, wt = _oracle(pcm, 6, 384000)
    got, gt = _gpu(engine, pcm, 6, 384000)
    assert np.array_equal(gt["mdct"], wt["mdct"]), "mdct_coef"
    assert np.array_equal(gt["exp_samples"], wt["shift"]), "exp_samples"
    assert np.array_equal(gt["exp_strategy"], wt["strat"]), "exp_strategy"
    assert np.array_equal(gt["snroffst"], wt["snr"]), (gt["snroffst"].tolist(), wt["snr"].tolist())
    for ch, n in [(0, 223), (1, 223), (2, 223), (3, 223), (4, 223), (5, 7)]:
        assert np.array_equal(gt["encoded_exp"][:, :, :, ch, :n], wt["encoded_exp"][:, :, :, ch, :n]), "encoded_exp %d" % ch
        assert np.array_equal(gt["bap"][:, :, :, ch, :n], wt["bap"][:, :, :, ch, :n]), "bap %d" % ch
    assert np.array_equal(got, want), "bitstream differs in %d bytes" % int((got != want).sum())


@pytest.mark.parametrize("nch,bitrate,freq", [(2, 192000, 48000), (1, 96000, 48000), (5, 448000, 48000), (3, 256000, 48000),
                                              (4, 320000, 48000), (6, 640000, 48000), (2, 128000, 32000),
                                              (2, 160000, 44100), (1, 48000, 24000), (6, 448000, 48000)])
def test_encode_other_configurations(engine, nch, bitrate, freq):
    """Every channel count AC3_encode_init accepts (acmod table :1029-1045), other bit rates, sample rates
    (incl. a half-rate bsid 9 stream) - and the stereo bit-budget overshoot quirk (:1609-1613)."""
    chmap = H.CHMAP6 if nch == 6 else tuple(range(8))
    pcm = [H.gen_pcm(4, nch, seed=5 + s, kind=("music", "tones", "noise")[s % 3]) for s in range(3)]
    want, _ = _oracle(pcm, nch, bitrate, freq, chmap)
    got, _ = _gpu(engine, pcm, nch, bitrate, freq, chmap, taps=False)
    bad = [(s, f, int((got[s, f] != want[s, f]).sum()), int(np.nonzero(got[s, f] != want[s, f])[0][0]))
           for s in range(got.shape[0]) for f in range(got.shape[1]) if not np.array_equal(got[s, f], want[s, f])]
    assert not bad, "frames (stream, frame, bytes differing, first byte): %r" % bad


def test_encode_state_carries_across_calls(engine):
    """last_samples and csnroffst (ac3enc.cpp:55,67,921,969) persist: two calls == one call."""
    pcm = [H.gen_pcm(6, 6, seed=77 + s, kind="tones") for s in range(3)]
    want, _ = _oracle(pcm, 6, 384000)
    got, _ = _gpu(engine, pcm, 6, 384000, taps=False, split=2)
    assert np.array_equal(got, want)


def test_encode_rejects_bad_parameters(engine):
    pkg = H.pkg()
    for args in ((48000, 384000, 0), (48000, 384000, 7), (47999, 384000, 6), (48000, 383000, 6)):
        assert pkg.EncodeDesc(*args).frame_bytes() == 0
    assert pkg.EncodeDesc(48000, 384000, 6).frame_bytes() == 1536


def test_host_tables_match_oracle(engine):
    """The Q15 tables are built on the host with cosf/sinf (fft_init, ac3enc.cpp:441-459,1098-1102)."""
    L = H.orc()
    pkg = H.pkg()
    lib = pkg.load_library()
    cos, sin, xc, xs, win = (np.zeros(n, np.int16) for n in (64, 64, 128, 128, 256))
    lib.ac3mi_encode_tables(cos.ctypes.data, sin.ctypes.data, xc.ctypes.data, xs.ctypes.data, win.ctypes.data)
    ocos, osin, oxc, oxs = (np.zeros(n, np.int16) for n in (64, 64, 128, 128))
    crc = np.zeros(256, np.uint16)
    L.orc_ac3enc_tables(H.P(ocos, H.i16p), H.P(osin, H.i16p), H.P(oxc, H.i16p), H.P(oxs, H.i16p), H.P(crc, H.u16p))
    assert np.array_equal(cos, ocos) and np.array_equal(sin, osin) and np.array_equal(xc, oxc) and np.array_equal(xs, oxs)


@pytest.mark.parametrize("kind", ["bursts", "strobe", "tones"])
def test_encode_second_generation_content(engine, kind):
    """Decoded AC-3 fed back to the encoder.  Its level steps inside runs of exponent reuse pull encoded exponents
    below a block's normalisation shift, where sym_quant's `c << e` (ac3enc.cpp:1150-1166) has a negative count: the
    engine and the oracle both restate what the x86 build executes (masked shift count, wrap-around multiply, unmasked
    put_bits), so the bitstreams still have to agree byte for byte."""
    L = H.orc()
    pcm2 = []
    for s in range(4):
        first = H.orc_encode(H.gen_pcm(3, 6, seed=500 + s, kind=kind))
        dec, errs, oflags = H.orc_decode(first, 7 | 16 | 32, 1.0, 384.0)
        assert errs == 0
        s16 = np.zeros((3 * 6, 256, 6), np.int16)
        for f in range(3):
            for b in range(6):
                L.orc_convert_s16(H.P(np.ascontiguousarray(dec[f, b]), H.fp), H.P(s16[f * 6 + b], H.i16p), oflags)
        pcm2.append(s16.reshape(3 * 1536, 6))
    want, _ = _oracle(pcm2, 6, 384000)
    got, _ = _gpu(engine, pcm2, 6, 384000, taps=False)
    bad = [(s, f, int((got[s, f] != want[s, f]).sum())) for s in range(4) for f in range(3) if not np.array_equal(got[s, f], want[s, f])]
    assert not bad, bad


@pytest.mark.parametrize("marker", [26, 60, 62, 120])
@pytest.mark.parametrize("kind,frames", [("tones", 3), ("bursts", 3), ("noise", 1)])
def test_grouped_code_equal_to_the_merged_marker_is_not_written(engine, kind, frames, marker):
    """ac3enc marks the slots of merged group members with 128 and its second pass skips every slot that holds 128
    (ac3enc.cpp:1375-1413, 1466-1480): an opener whose (out-of-contract, garbage) 16-bit code equals 128 is not written
    and the rest of the block moves up by 5 or 7 bits.  Content that produces such a code is practically impossible to
    make (12 000 negative-shift quantisations of second-generation material: none), so the mechanism is exercised with
    the marker moved to a value ordinary codes take - the same knob in the oracle (orc_ac3enc_set_marker) and in the
    engine (AC3MI_ENC_MARKER, read per launch): dozens of dropped fields per frame, byte-exact streams."""
    import ctypes
    import os
    L = H.orc()
    L.orc_ac3enc_set_marker.argtypes = [ctypes.c_int]
    L.orc_ac3enc_debug_counts.argtypes = [ctypes.POINTER(ctypes.c_long)] * 2
    pcm = [H.gen_pcm(frames, 6, seed=40 + s, kind=kind) for s in range(3 if frames > 1 else 7)]      # (one-frame streams: the unsplit pack kernel)
    plain, _ = _oracle(pcm, 6, 384000)
    c0 = ctypes.c_long()
    L.orc_ac3enc_debug_counts(ctypes.byref(c0), None)
    L.orc_ac3enc_set_marker(marker)
    os.environ["AC3MI_ENC_MARKER"] = str(marker)
    try:
        want, _ = _oracle(pcm, 6, 384000)
        got, _ = _gpu(engine, pcm, 6, 384000, taps=False)
    finally:
        L.orc_ac3enc_set_marker(128)
        del os.environ["AC3MI_ENC_MARKER"]
    c1 = ctypes.c_long()
    L.orc_ac3enc_debug_counts(ctypes.byref(c1), None)
    if c1.value == c0.value:
        pytest.skip("this content has no code equal to %d" % marker)
    assert not np.array_equal(want, plain)                                     # fields were dropped
    assert np.array_equal(got, want), "bitstream differs in %d bytes" % int((got != want).sum())
    again, _ = _gpu(engine, pcm, 6, 384000, taps=False)                       # and the default is back
    assert np.array_equal(again, plain)


@pytest.mark.parametrize("kind", ["silence", "rails", "impulses", "dc"])
@pytest.mark.parametrize("nch,bitrate", [(6, 384000), (2, 192000), (1, 64000)])
def test_encode_extreme_levels(engine, kind, nch, bitrate):
    """Digital silence, full-scale squares / DC / impulses including -32768: the corners of the fixed-point transform
    (int16 wrap in the FFT butterflies, abs(-32768), normalisation shift 0 and 16: ac3enc.cpp:493-611, 1673-1697),
    exponent 24 everywhere and the SNR-offset search running into both of its ends (:921-967).  Byte-exact, and the
    frames decode on the GPU to what liba52's restatement makes of them."""
    chmap = H.CHMAP6 if nch == 6 else tuple(range(8))
    pcm = [H.gen_pcm(3, nch, seed=70 + s, kind=kind) for s in range(2)]
    want, wt = _oracle(pcm, nch, bitrate, 48000, chmap)
    got, gt = _gpu(engine, pcm, nch, bitrate, 48000, chmap)
    assert np.array_equal(gt["mdct"], wt["mdct"][..., :nch, :]), "mdct_coef"
    assert np.array_equal(gt["snroffst"], wt["snr"]), (gt["snroffst"].tolist(), wt["snr"].tolist())
    assert np.array_equal(got, want), "bitstream differs in %d bytes" % int((got != want).sum())
    from tests import test_decode_gpu as D
    n, sflags, _, _ = H.pkg().syncinfo(got[0, 0])
    ref_pcm, _, ref_lfsr, _ = D._oracle_decode_with_taps(got, sflags & 0x1f, 1.0, 0.0)
    dec, status, _, lfsr = D._gpu_decode(engine, got, sflags & 0x1f, 1.0, 0.0, taps=False)
    assert (status & 0x1ff).max() == 0 and np.array_equal(lfsr, ref_lfsr)
    assert H.rms(dec.astype(np.float64) - ref_pcm) <= 1e-6


def test_starved_bit_rate_is_survivable(engine):
    """6 channels of noise at 64 kbps: AC3_encode_init accepts it, but not even csnroffst 0 fits the frame, the
    reference prints "Yack, Error !!!" (ac3enc.cpp:930-933), keeps going with stale offsets and writes past the frame
    size (what lands inside the frame is recorded in tests/golden/ac3enc_ref.npz, stream "51_starved", and compared in
    tests/test_encode_ref_gpu.py).  Here: the engine must stay inside its buffers, produce a frame-sized output with a
    header, leave neighbours alone and keep working: a stream with the same samples at 384 kbps, encoded right after with
    the same context, is still byte-exact."""
    import torch
    pkg = H.pkg()
    S, F = 3, 2
    pcm = [H.gen_pcm(F, 6, seed=880 + s, kind="noise") for s in range(S)]
    desc = pkg.EncodeDesc(48000, 64000, 6)
    fb = desc.frame_bytes()
    assert fb == 256
    t = torch.from_numpy(np.stack(pcm).reshape(S, F, 1536, 6)).cuda()
    last = torch.zeros((S, 6, 256), dtype=torch.int16, device="cuda")
    csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
    guard = torch.full((S, F, fb + 64), 0xA5, dtype=torch.uint8, device="cuda")       # 64 guard bytes behind every frame
    out = engine.encode_batch(desc, t, H.CHMAP6, last, csnr, out=guard)
    engine.sync()
    o = out.cpu().numpy()
    assert (o[:, :, 0] == 0x0b).all() and (o[:, :, 1] == 0x77).all()
    assert (o[:, :, fb:] == 0xA5).all(), "wrote past the frame"
    assert (csnr.cpu().numpy() == 40).all()          # a failed search leaves the stream's start value alone (:921-933)
    want, _ = _oracle(pcm, 6, 384000)
    got, _ = _gpu(engine, pcm, 6, 384000, taps=False)
    assert np.array_equal(got, want)


def test_failed_search_follows_the_reference(engine):
    """3 channels at 48 kbps / 24 kHz: the previous frame's csnroffst (3) does not fit the next frame and 3 - 4 is negative,
    so the reference's search gives up ("Yack, Error !!!", ac3enc.cpp:921-933) although csnroffst 0..2 would fit:
    compute_bit_allocation returns without storing offsets, its caller carries on (:1752) - the header repeats the previous
    frame's offsets, the mantissas follow the allocation of the last attempt.  Found by tests/fuzz_encode.py (seed 101,
    round 25).  The engine matches the oracle byte for byte on both batch-shape paths, and the search state it hands back
    (csnroffst | fsnroffst << 8) lets the next call continue the same way."""
    import torch
    pkg = H.pkg()
    nch, freq, bitrate = 3, 24000, 48000
    chmap = tuple(range(8))
    pcm = [H.gen_pcm(4, nch, seed=101000 + 25 * 7 + s, kind=k) for s, k in enumerate(("music", "tones", "tones", "music"))]
    want, wt = _oracle(pcm, nch, bitrate, freq, chmap)
    got, gt = _gpu(engine, pcm, nch, bitrate, freq, chmap)
    snr = wt["snr"].reshape(4, 4, 2)
    assert np.array_equal(gt["snroffst"].reshape(4, 4, 2), snr)
    assert np.array_equal(snr[0, 3], snr[0, 2]) and np.array_equal(snr[3, 2], snr[3, 1])     # the two frames that repeat stale offsets
    assert np.array_equal(got, want), "bitstream differs in %d bytes" % int((got != want).sum())
    # frame by frame, the state carried by the caller
    desc = pkg.EncodeDesc(freq, bitrate, nch)
    x = torch.from_numpy(np.stack(pcm).reshape(4, 4, 1536, nch)).cuda()
    last = torch.zeros((4, nch, 256), dtype=torch.int16, device="cuda")
    csnr = torch.full((4,), 40, dtype=torch.int32, device="cuda")
    parts = []
    for f in range(4):
        out = engine.encode_batch(desc, x[:, f:f + 1].contiguous(), chmap[:nch], last, csnr)
        engine.sync()
        parts.append(out.cpu().numpy()[:, :, :want.shape[2]])
    assert np.array_equal(np.concatenate(parts, axis=1), want)
    st = csnr.cpu().numpy()
    assert np.array_equal(st & 0xff, snr[:, 3, 0]) and np.array_equal((st >> 8) & 15, snr[:, 3, 1])


def test_batch_shape_paths_agree(engine):
    """One call with six frames per stream goes through the tabulate / replay / pack-per-frame kernels; six calls of one
    frame each go through the one-wavefront-per-stream kernel with the state carried by the caller.  Same bytes."""
    import torch
    pkg = H.pkg()
    S, F = 8, 6
    pcm = [H.gen_pcm(F, 6, seed=640 + s, kind=("bursts", "tones", "strobe", "music", "noise", "quiet", "bursts", "tones")[s]) for s in range(S)]
    desc = pkg.EncodeDesc(48000, 384000, 6)
    x = torch.from_numpy(np.stack(pcm).reshape(S, F, 1536, 6)).cuda()
    last = torch.zeros((S, 6, 256), dtype=torch.int16, device="cuda")
    csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
    with V.tap(engine) as whole_log:
        whole = engine.encode_batch(desc, x, H.CHMAP6, last, csnr)
        engine.sync()
    last1 = torch.zeros((S, 6, 256), dtype=torch.int16, device="cuda")
    csnr1 = torch.full((S,), 40, dtype=torch.int32, device="cuda")
    parts = []
    with V.tap(engine) as step_log:
        for f in range(F):
            parts.append(engine.encode_batch(desc, x[:, f:f + 1].contiguous(), H.CHMAP6, last1, csnr1))
            engine.sync()
    step = torch.cat(parts, dim=1)
    # the routes the name speaks of were taken (ac3mi_debug_launch_log): the tabulating search in the whole call alone
    assert V.search(3) in whole_log and V.search(1) in whole_log, whole_log
    assert len(step_log) == 3 * F and not any(k.startswith("enc_search_kernel<3") for k in step_log), step_log
    assert torch.equal(whole.cpu(), step.cpu())
    assert torch.equal(last.cpu(), last1.cpu()) and torch.equal(csnr.cpu(), csnr1.cpu())
    want, _ = _oracle(pcm, 6, 384000)
    assert np.array_equal(whole.cpu().numpy()[:, :, :1536], want)


@pytest.mark.parametrize("nch,bitrate,freq", [(6, 384000, 48000), (2, 192000, 44100), (1, 96000, 32000), (3, 48000, 24000)])
def test_block_packer_equals_the_stream_packer(engine, nch, bitrate, freq):
    """ac3mi_set_encode_mode: 1 = one wavefront per stream searches and packs (per frame for few long streams), 2 = searches
    per stream, then six wavefronts per frame - one per audio block - pack at once from bit counts.  Same frames, same
    carry-over state, same bap taps, on one-frame and on multi-frame streams (the last configuration starves: frames whose
    search fails, ENC/ac3enc.cpp:930-933)."""
    import os
    import torch
    pkg = H.pkg()
    desc = pkg.EncodeDesc(freq, bitrate, nch)
    chmap = H.CHMAP6[:nch] if nch == 6 else tuple(range(nch))
    for S, F in ((9, 1), (3, 5)):
        pcm = torch.from_numpy(np.stack([H.gen_pcm(F, nch, seed=400 + 7 * s + nch, kind=("bursts", "music", "quiet", "noise", "strobe")[s % 5])
                                         for s in range(S)]).reshape(S, F, 1536, nch)).cuda()
        res = {}
        try:
            for mode in (1, 2):
                engine.set_encode_mode(mode)
                last = torch.zeros((S, nch, 256), dtype=torch.int16, device="cuda")
                csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
                with V.tap(engine) as log:
                    frames, taps = engine.encode_batch(desc, pcm, chmap, last, csnr, taps=True)
                    engine.sync()
                # mode 1 packed with one wavefront per frame, mode 2 with one per audio block
                assert ("enc_packf_kernel" if mode == 1 else "enc_packb_kernel") in V.families(log), (mode, log)
                assert ("enc_packb_kernel" if mode == 1 else "enc_packf_kernel") not in V.families(log), (mode, log)
                res[mode] = [x.cpu().numpy() for x in (frames, last, csnr, taps["bap"], taps["snroffst"], taps["exp_strategy"])]
        finally:
            engine.set_encode_mode(int(os.environ.get("AC3MI_ENCODE_MODE", "0")))
        for a, b in zip(res[1], res[2]):
            assert np.array_equal(a, b), (S, F)
