"""CPU: tests/ac3_syntax.py, the independent A/52 frame reader and bit counter, proven against what is already pinned.

* packer streams (every acmod x LFE, three sample rates, bsid 8 / 9 / 10, coupling, delta allocation, skip fields, block
  switching): block end positions, exponents and bap equal the decode oracle's, which is pinned bit for bit to the real
  liba52 on exactly these streams (test_packer_streams.py);
* oracle-encoded streams (1..6 channels, the rates of test_encode_other_configurations, first- and second-generation
  content): the same three equalities, bap equal to the encoder oracle's, offsets equal to its header's;
* the reader's spare-bit curve equals the encoder oracle's at all 1024 offsets, with c = 4 uncounted bits in 2/0 frames and
  0 elsewhere: search_allocation (ENC/ac3enc.cpp:880-916, restated in oracle/ac3enc_oracle.c) prices one bit of rematstr
  per block where block 0 writes rematstr and four flags;
* the reference's search loop replayed on the reader's curve ends at the offsets the oracle coded, frame after frame.
Every comparison is an integer equality."""
import ctypes
import os
import sys

import numpy as np
import pytest

from tests import _harness as H
from tests import ac3_syntax as A
from tests import packer

sys.path.insert(0, os.path.join(H.ROOT, "profiles"))
import search_sim                                       # noqa: E402

LIBA52_CODE = np.array([0, -1, -2, 3, -3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16], np.int8)   # liba52's names for bap 0..15

ENC_CONFIGS = [(2, 192000, 48000), (1, 96000, 48000), (5, 448000, 48000), (3, 256000, 48000), (4, 320000, 48000),
               (6, 640000, 48000), (2, 128000, 32000), (2, 160000, 44100), (1, 48000, 24000), (6, 448000, 48000),
               (6, 384000, 48000)]
ACMOD_OF_NCH = {1: 1, 2: 2, 3: 3, 4: 6, 5: 7, 6: 7}


def check_against_decoder(frames, acmod, lfeon):
    """frames [F][fb] of one stream: reader against the decode oracle, block by block.  Returns the parsed frames."""
    L = H.orc()
    nfr, fb = frames.shape
    buf = np.zeros(nfr * fb + 64, np.uint8)
    buf[:nfr * fb] = frames.reshape(-1)
    st = L.orc_a52_init()
    out = []
    for f in range(nfr):
        fr = A.parse_frame(frames[f])
        assert fr.frame_bytes == fb and fr.acmod == acmod and fr.lfeon == lfeon
        fl, lv = H.ci(acmod | (16 if lfeon else 0)), H.cf(1.0)
        assert L.orc_a52_frame(st, ctypes.cast(buf.ctypes.data + f * fb, H.u8p), ctypes.byref(fl), ctypes.byref(lv), 0.0) == 0
        for b, B in enumerate(fr.blocks):
            assert L.orc_a52_block(st) == 0
            assert L.orc_a52_bitpos(st) == B.end, "frame %d block %d ends at %d, the reader says %d" % (f, b, L.orc_a52_bitpos(st), B.end)
            assert B.end - B.start == B.side_bits + B.mant_bits
            for r, (s, e) in B.rng.items():
                ex, bp = np.zeros(256, np.uint8), np.zeros(256, np.int8)
                L.orc_a52_get_exp(st, r, H.P(ex, H.u8p))
                L.orc_a52_get_bap(st, r, H.P(bp, H.i8p))
                assert np.array_equal(ex[s:e], B.exp[r, s:e]), "exponents, frame %d block %d row %d" % (f, b, r)
                assert np.array_equal(bp[s:e], LIBA52_CODE[B.bap[r, s:e]]), "bap, frame %d block %d row %d" % (f, b, r)
        out.append(fr)
    L.orc_a52_free(st)
    return out


PACKER_SHAPES = [(0, 8, 36), (1, 8, 37), (2, 10, 30), (0, 9, 36), (1, 9, 36), (2, 9, 30), (0, 10, 36), (1, 10, 37), (2, 8, 30)]


@pytest.mark.parametrize("acmod", range(8))
@pytest.mark.parametrize("lfe", [0, 1])
def test_reader_equals_liba52_on_packer_streams(acmod, lfe):
    seen = dict(cpl=0, delta=0, skip=0, blksw=0, remat=0, dynrng=0, blocks=0)
    for fscod, bsid, fsz in PACKER_SHAPES:
        fr = packer.make_stream(31337 + acmod * 2 + lfe + fscod * 100 + bsid, 3, acmod, lfe, fscod=fscod, bsid=bsid, frmsizecod=fsz)
        for P in check_against_decoder(fr, acmod, lfe):
            assert P.fscod == fscod and P.bsid == bsid and P.fields["frmsizecod"] == fsz
            for B in P.blocks:
                seen["blocks"] += 1
                seen["cpl"] += A.CPL in B.rng
                seen["delta"] += any(k.startswith("deltoffst") for k in B.fields)
                seen["skip"] += B.fields["skiple"]
                seen["blksw"] += any(B.fields["blksw%d" % c] for c in range(P.nfchans))
                seen["remat"] += any(v for k, v in B.fields.items() if k.startswith("rematflg"))
                seen["dynrng"] += B.fields["dynrnge"]
    assert seen["blocks"] == len(PACKER_SHAPES) * 18
    assert seen["delta"] > 10 and seen["skip"] > 10 and seen["blksw"] > 10 and seen["dynrng"] > 10, seen
    assert (seen["cpl"] > 10) == (acmod >= 2) and (seen["remat"] > 10) == (acmod == 2), seen


def test_every_bsi_option_is_read():
    """compr, langcod, audprodi (both programmes), both time codes and addbsi all occur in the sweep's dual-mono streams and
    the reader still lands on the decoder's positions (a skipped optional field would move every block)."""
    names = set()
    for seed in range(12):
        fr = packer.make_stream(900 + seed, 2, 0, seed & 1)
        for P in check_against_decoder(fr, 0, seed & 1):
            names |= {k for k, v in P.fields.items() if k.endswith("e") and v}
    assert {"compre", "langcode", "audprodie", "compr2e", "langcod2e", "audprodi2e", "timecod1e", "timecod2e", "addbsie"} <= names


def oracle_encode(pcm, nch, bitrate, freq, chmap, curve=True):
    """One stream through the encoder oracle -> frames [F][fb], per frame its bap [6][6][256], encoded exponents, header
    offsets (csnroffst, fsnroffst) and its spare-bit curve [1024]."""
    L = H.orc()
    L.orc_ac3enc_set_spare_curve.argtypes = [ctypes.c_void_p]
    F = pcm.shape[0] // 1536
    fb = H.ci()
    h = L.orc_ac3enc_init(freq, bitrate, nch, ctypes.byref(fb))
    assert h
    frames = np.zeros((F, fb.value), np.uint8)
    cm = (ctypes.c_uint8 * 8)(*chmap)
    pcm = np.ascontiguousarray(pcm)
    buf = np.zeros(1024, np.int32)
    baps, exps, snr, curves = [], [], [], []
    L.orc_ac3enc_set_spare_curve(buf.ctypes.data if curve else None)
    try:
        for f in range(F):
            assert L.orc_ac3enc_frame(h, H.P(frames[f], H.u8p), ctypes.cast(pcm.ctypes.data + f * 1536 * nch * 2, H.i16p), cm) == fb.value
            b, e1, e2 = (np.zeros((6, 6, 256), np.uint8) for _ in range(3))
            st, sh = np.zeros((6, 6), np.uint8), np.zeros((6, 6), np.int8)
            c, fs = H.ci(), H.ci()
            L.orc_ac3enc_get_bap(h, H.P(b, H.u8p))
            L.orc_ac3enc_get_exp(h, H.P(e1, H.u8p), H.P(e2, H.u8p))
            L.orc_ac3enc_get_misc(h, H.P(st, H.u8p), H.P(sh, H.i8p), ctypes.byref(c), ctypes.byref(fs))
            baps.append(b)
            exps.append(e2)
            snr.append((c.value, fs.value))
            curves.append(buf.copy())
    finally:
        L.orc_ac3enc_set_spare_curve(None)
        L.orc_ac3enc_free(h)
    return frames, baps, exps, snr, curves


def second_generation(pcm, nch, bitrate, freq, chmap):
    """the stream encoded, decoded to s16 at bias 384 and handed back in the encoder's input order"""
    L = H.orc()
    first = H.orc_encode(pcm, nch, bitrate, freq, chmap)
    lfe = nch == 6
    flags = ACMOD_OF_NCH[nch] | (16 if lfe else 0) | 32
    dec, errs, oflags = H.orc_decode(first, flags, 1.0, 384.0)
    assert errs == 0
    F = first.shape[0]
    s16 = np.zeros((F * 6, 256, nch), np.int16)
    for f in range(F):
        for b in range(6):
            L.orc_convert_s16(H.P(np.ascontiguousarray(dec[f, b]), H.fp), H.P(s16[f * 6 + b], H.i16p), oflags)
    return s16.reshape(F * 1536, nch)


def check_oracle_stream(pcm, nch, bitrate, freq):
    chmap = H.CHMAP6 if nch == 6 else tuple(range(8))
    frames, baps, exps, snr, curves = oracle_encode(pcm, nch, bitrate, freq, chmap)
    acmod, lfe = ACMOD_OF_NCH[nch], int(nch == 6)
    parsed = check_against_decoder(frames, acmod, lfe)
    c = 4 if acmod == 2 else 0
    start = 40
    for f, P in enumerate(parsed):
        assert A.uncounted_bits(P) == c
        for b, B in enumerate(P.blocks):
            assert B.csnroffst == snr[f][0] and set(B.fsnroffst.values()) == {snr[f][1]}
            for k, r in enumerate(P.rows()):
                s, e = B.rng[r]
                assert np.array_equal(B.bap[r, s:e], baps[f][b, k, s:e]), "bap, frame %d block %d row %d" % (f, b, r)
                assert np.array_equal(B.exp[r, s:e], exps[f][b, k, s:e]), "exponents, frame %d block %d row %d" % (f, b, r)
        # the frame as coded spends what the curve says at its own offsets
        g = 16 * snr[f][0] + snr[f][1]
        assert A.spent_bits(P, g) == P.side_bits + sum(P.mant_bits) == P.blocks[5].end
        mine = np.array([8 * P.frame_bytes - 18 - A.spent_bits(P, k) + c for k in range(1024)])
        bad = np.nonzero(mine != curves[f])[0]
        assert bad.size == 0, "spare bits differ at %d offsets, first g = %d: reader %d, oracle %d" % (
            bad.size, bad[0], mine[bad[0]], curves[f][bad[0]])
        got = search_sim.reference(A.SpareCurve(P, c), start)
        assert got == snr[f], "frame %d: the replayed search ends at %r, the oracle coded %r" % (f, got, snr[f])
        start = snr[f][0]


@pytest.mark.parametrize("nch,bitrate,freq", ENC_CONFIGS)
def test_reader_on_oracle_encoded_streams(nch, bitrate, freq):
    for s, kind in enumerate(("music", "tones", "noise", "bursts")):
        check_oracle_stream(H.gen_pcm(3, nch, seed=5 + s, kind=kind), nch, bitrate, freq)


@pytest.mark.parametrize("nch,bitrate,freq", ENC_CONFIGS)
def test_reader_on_second_generation_streams(nch, bitrate, freq):
    chmap = H.CHMAP6 if nch == 6 else tuple(range(8))
    for s, kind in enumerate(("bursts", "tones")):
        pcm2 = second_generation(H.gen_pcm(3, nch, seed=500 + s, kind=kind), nch, bitrate, freq, chmap)
        check_oracle_stream(pcm2, nch, bitrate, freq)


def test_all_zero_offsets_mean_no_mantissas():
    """A frame whose offsets are all zero carries no mantissas (A/52 §5.4.3.37 - 40; liba52 parse.c zero_snr_offsets) - the
    reader follows that when it PARSES, while spent_bits(frame, 0) prices the formula's allocation as the reference's search
    does (it never codes g = 0 unless the formula's count fits)."""
    fr = H.orc_encode(H.gen_pcm(1, 2, seed=3, kind="music"), 2, 192000, 48000, tuple(range(8)))[0].copy()
    P = A.parse_frame(fr)
    bits = np.unpackbits(fr)
    B = P.blocks[0]
    for name, n in [("csnroffst", 6)] + [("fsnroffst%d" % c, 4) for c in range(2)]:
        bits[B.pos[name]:B.pos[name] + n] = 0
    Z = A.parse_frame(np.packbits(bits), nblocks=1)        # what follows block 0 is then misplaced
    assert Z.blocks[0].mant_bits == 0 and not Z.blocks[0].bap.any()
    assert sum(A.mantissa_bits_at(P, 0)) > 0


def test_matrix_rates_do_not_starve_the_plain_encoder():
    """The GPU audit (tests/test_frame_budget_gpu.py) excludes frames whose search fails and must therefore meet none: at
    its rates the plain encoder (the oracle, mode 0) does not fail on the same content, and at the lower rate of each
    channel count it does not saturate at csnroffst 63 on the matrix's six programmes (the DRC programme ends in silence)."""
    from tests import test_frame_budget_gpu as G
    from tests._tools import programme
    for nch in range(1, 7):
        chmap = H.CHMAP6 if nch == 6 else tuple(range(8))
        for sr in (48000, 44100):
            for hi in (0, 1):
                streams = list(G.matrix_content(nch)) + ([programme(nch, seed=11 + nch)[0]] if nch in (1, 2, 6) else [])
                for k, pcm in enumerate(streams):
                    _, _, _, snr, curves = oracle_encode(pcm, nch, G.RATES[nch][hi], sr, chmap)
                    start = 40
                    for f, curve in enumerate(curves):      # (the oracle returns a frame after a failed search too)
                        ss = search_sim.Search(start)
                        while True:
                            q = ss.next()
                            if q is None:
                                break
                            ss.consume(curve[16 * q[0] + q[1]] >= 0)
                        assert not ss.failed and (ss.c, ss.f) == snr[f], (nch, sr, hi, k, f)
                        assert curve[16 * snr[f][0] + snr[f][1]] >= 0
                        start = snr[f][0]
                    assert hi == 1 or k >= 6 or max(c for c, _ in snr) < 63, (nch, sr, snr)


def test_audit_helper_on_oracle_frames(monkeypatch):
    """The GPU audit's helper run here on the oracle's frames and taps (mode 0): it passes them; it reports a bap tap that
    is off in one bin and a header that disagrees with the offsets tap; and with 400 bits of room that do not exist (the
    uncounted constant inflated) the replayed search ends above the coded offsets and item 3 says so."""
    from tests import test_frame_budget_gpu as G
    for nch, rate in ((2, 96000), (6, 224000)):
        chmap = H.CHMAP6 if nch == 6 else tuple(range(8))
        pcm = H.gen_pcm(3, nch, seed=9, kind="tones")
        frames, baps, exps, snr, _ = oracle_encode(pcm, nch, rate, 48000, chmap, curve=False)
        taps = dict(snroffst=np.array(snr)[None], bap=np.array(baps)[None][:, :, :, :nch], encoded_exp=np.array(exps)[None][:, :, :, :nch])
        rep = G.Report()
        G.audit(rep, frames[None], taps, [40], "oracle")
        rep.finish("oracle frames")
        assert rep.n["frames"] == 3
        bad = {k: v.copy() for k, v in taps.items()}
        bad["bap"][0, 1, 2, 0, 5] ^= 1
        bad["snroffst"][0, 2, 1] ^= 1
        rep = G.Report()
        G.audit(rep, frames[None], bad, [40], "oracle")
        assert sorted(f.split(" | ")[0] for f in rep.fails) == ["bap", "syntax"], rep.fails
        with monkeypatch.context() as m:
            real = A.uncounted_bits
            m.setattr(A, "uncounted_bits", lambda P: real(P) + 400)
            rep = G.Report()
            G.audit(rep, frames[None], taps, [40], "oracle")
        assert rep.fails and {f.split(" | ")[0] for f in rep.fails} == {"search"}, rep.fails
