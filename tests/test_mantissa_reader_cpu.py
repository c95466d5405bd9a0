"""CPU: the tooling of the mantissa audit - tests/ac3_syntax.read_mantissas, tests/quantiser_model.py and
tests/mantissa_audit.py - proven against what is already pinned, before it judges the GPU encoder
(tests/test_tool_mantissas_gpu.py).

* reader and model against the encoder oracle (pinned byte for byte to the reference's ac3enc): every coded bin of its
  frames carries the code the model makes of the oracle's own mdct / shift stage arrays; no bin is left out on
  first-generation content, and the reader's bap is the oracle's;
* second-generation content, where reuse runs pull exponents below a block's shift: the in-contract bins still agree, every
  bin left out has a negative e, and the symmetric ones among the bins with a negative e are exactly what the oracle's own
  counter counted (it sits in front of quant_sym only: a bap of 6 and up with a negative e is left out here and is not
  counted there);
* the reader against liba52's restatement (the decode oracle, pinned bit for bit to liba52): order, grouping and field
  widths, independently of any encoder, on packer streams with coupling, block switching and delta bit allocation;
* the audit notices: one flipped mantissa bit and two swapped fields are reported at exactly their bins.
Every comparison is an integer (or float-bit) equality except the coupled bins of the third item."""
import ctypes

import numpy as np
import pytest

from tests import _harness as H
from tests import ac3_syntax as A
from tests import mantissa_audit as MA
from tests import packer
from tests import quantiser_model as Q
from tests.test_encode_gpu import _oracle
from tests.test_frame_budget_gpu import RATES, matrix_content
from tests.test_packer_quantiser_gpu import _negshift_count, _second_generation

# (channels, bit rate, sample rate); the fourth is starved: csnroffst 2..7.  (A frame whose search fails is no AC-3 frame -
# the reference writes its last attempt over the frame's end - and has nothing to audit: the seeds below give none.)
CONFIGS = [(6, 384000, 48000), (2, 192000, 48000), (1, 96000, 44100), (3, 48000, 24000), (5, 448000, 32000)]
KINDS = ("music", "bursts", "quiet", "noise")


def oracle_audit(rep, pcm, nch, rate, freq, label):
    """encode with the oracle, audit its frames against its own stage arrays; -> (frames, taps)"""
    chmap = H.CHMAP6 if nch == 6 else tuple(range(8))
    frames, t = _oracle(pcm, nch, rate, freq, chmap)
    S, F = frames.shape[:2]
    nf, lfe = min(nch, 5), int(nch == 6)
    rs = [[MA.frame_rows(t["mdct"][s, f], t["shift"][s, f], nf, lfe) for f in range(F)] for s in range(S)]
    parsed = [[None] * F for _ in range(S)]
    MA.audit_mantissas(rep, frames, [[x[0] for x in r] for r in rs], [[x[1] for x in r] for r in rs], label, parsed)
    for s in range(S):
        for f in range(F):
            P = parsed[s][f]
            for b, B in enumerate(P.blocks if P else ()):
                for k, r in enumerate(P.rows()):
                    lo, hi = B.rng[r]
                    if not np.array_equal(B.bap[r, lo:hi], t["bap"][s, f, b, k, lo:hi]):
                        rep.fail("bap", "%s stream %d frame %d" % (label, s, f), "block %d row %d: the reader's bap is not the oracle's" % (b, r))
    return frames, t


@pytest.mark.parametrize("nch,rate,freq", CONFIGS)
def test_oracle_frames_carry_the_models_codes(nch, rate, freq):
    rep = MA.Report()
    pcm = [H.gen_pcm(3, nch, seed=31 + i, kind=k) for i, k in enumerate(KINDS)]
    oracle_audit(rep, pcm, nch, rate, freq, "%d ch %d b/s %d Hz" % (nch, rate, freq))
    rep.finish("oracle, %d channels at %d b/s, %d Hz" % (nch, rate, freq))
    assert rep.n["frames"] == 12 and rep.n["compared"] > 0 and rep.n["left_out"] == 0, rep.n


@pytest.mark.parametrize("hi", [0, 1])
@pytest.mark.parametrize("nch", [1, 2, 6])
def test_oracle_frames_of_the_matrix_content(nch, hi):
    """the content of the GPU matrix at its rates: the reference encoder leaves no bin out of contract on it"""
    rep = MA.Report()
    oracle_audit(rep, list(matrix_content(nch)), nch, RATES[nch][hi], 48000, "matrix %d ch" % nch)
    rep.finish("oracle on the matrix content, %d channels at %d b/s" % (nch, RATES[nch][hi]))
    assert rep.n["frames"] == 18 and rep.n["compared"] > 0 and rep.n["left_out"] == 0, rep.n


def test_second_generation_content():
    rep = MA.Report()
    counted = sym_neg = any_neg = 0
    for kind in ("bursts", "strobe", "music"):
        pcm = _second_generation(range(800, 806), kind, 3)
        n0 = _negshift_count()
        frames, t = oracle_audit(rep, pcm, 6, 384000, 48000, "second generation " + kind)
        counted += _negshift_count() - n0
        for s in range(frames.shape[0]):
            for f in range(frames.shape[1]):
                P = A.parse_frame(frames[s, f])
                for b, B in enumerate(P.blocks):
                    for k, r in enumerate(P.rows()):
                        lo, hi = B.rng[r]
                        neg = (B.exp[r, lo:hi].astype(np.int64) < int(t["shift"][s, f, b, k])) & (B.bap[r, lo:hi] > 0)
                        sym_neg += int((neg & (B.bap[r, lo:hi] <= 5)).sum())
                        any_neg += int((neg & (t["mdct"][s, f, b, k, lo:hi] != 0)).sum())
    rep.finish("oracle on second-generation content")
    print("second generation: %d bins out of contract; %d coded bins with a negative e and a symmetric bap, the oracle counted %d" % (
        rep.n["left_out"], sym_neg, counted))
    assert rep.n["compared"] > 100000
    assert sym_neg == counted > 0                       # the oracle's counter sits in quant_sym's path only
    assert rep.n["left_out"] == any_neg > 0             # and nothing is out of contract for another reason than e < 0


# ---------------------------------------------------------------------------------------------------------------------
# the reader against liba52's restatement

def _q(num, den):
    """liba52/tables.h:49 - Q(x) = ROUND(32768.0 * num / den), as float32"""
    x = 32768.0 * num / den
    return np.float32(int(x + (0.5 if x > 0 else -0.5)))


LEVEL = {b: np.array([_q(2 * (i - n // 2), n) for i in range(n)], np.float32) for b, n in A.SYM_LEVELS.items()}
WIDTH = dict(Q.ASYM_BITS)


def dequantised(code, bap, exp):
    """liba52's value of one mantissa code at an exponent, at level 1 and without dynrng (parse.c:345-433): the level
    constant, or the signed field << (16 - width), times scale_factor[exp] = 2^-(15 + exp), times the gain 2 that a52_frame
    makes of level 1 (parse.c:168-169): exact in float32"""
    if bap in LEVEL:
        m = float(LEVEL[bap][code])
    else:
        w = WIDTH[bap]
        m = float((code - (1 << w) if code >> (w - 1) else code) << (16 - w))
    return np.float32(np.ldexp(m, -(14 + int(exp))))


@pytest.mark.parametrize("acmod", [7, 3, 1])
@pytest.mark.parametrize("lfe", [0, 1])
def test_reader_equals_liba52_on_packer_streams(acmod, lfe):
    L = H.orc()
    L.orc_a52_get_coefs.argtypes = [H.vp, H.fp, H.u8p]
    nf = A.NFCHANS[acmod]
    n = dict(exact=0, coupled=0, bad=0, dither=0, cpl_blocks=0, short=0, delta=0)
    for seed in range(4):
        fr = packer.make_stream(5150 + 16 * seed + 2 * acmod + lfe, 3, acmod, lfe,
                                features=dict(cpl=0.8, blksw=0.4, deltba=0.6))
        nfr, fb = fr.shape
        buf = np.zeros(nfr * fb + 64, np.uint8)
        buf[:nfr * fb] = fr.reshape(-1)
        st = L.orc_a52_init()
        for f in range(nfr):
            P = A.parse_frame(fr[f])
            mant = A.read_mantissas(fr[f], P)
            fl, lv = H.ci(acmod | (16 if lfe else 0)), H.cf(1.0)
            assert L.orc_a52_frame(st, ctypes.cast(buf.ctypes.data + f * fb, H.u8p), ctypes.byref(fl), ctypes.byref(lv), 0.0) == 0
            assert fl.value == acmod | (16 if lfe else 0)
            L.orc_a52_dynrng(st, None, None)
            strc, co = [], {}
            for b, (B, M) in enumerate(zip(P.blocks, mant)):
                assert L.orc_a52_block(st) == 0
                plane, sw = np.zeros((6, 256), np.float32), np.zeros(5, np.uint8)
                L.orc_a52_get_coefs(st, H.P(plane, H.fp), H.P(sw, H.u8p))
                n["short"] += int(sw[:nf].any())
                n["delta"] += any(k.startswith("deltoffst") for k in B.fields)
                # the coupling state a decoder carries from block to block (A/52 5.4.3.7 - 5.4.3.18)
                if B.fields["cplstre"] and B.cplinu:
                    strc = [B.fields["cplbndstrc%d" % sb] for sb in range(1, 3 + B.cplendf - B.cplbegf)]
                for ch in range(nf):
                    if B.cplinu and B.chincpl[ch] and B.fields.get("cplcoe%d" % ch):
                        master = 3 * B.fields["mstrcplco%d" % ch]
                        co[ch] = []
                        for bnd in range(B.ncplbnd):
                            ex, ma = B.fields["cplcoexp%d_%d" % (ch, bnd)], B.fields["cplcomant%d_%d" % (ch, bnd)]
                            ma = ma << 14 if ex == 15 else (ma | 0x10) << 13
                            co[ch].append(np.ldexp(float(ma), -(15 + ex + master)))       # A/52 7.4.3, in liba52's scaling
                for r, (lo, hi) in B.rng.items():
                    for k in range(lo, hi):
                        bap = int(B.bap[r, k])
                        if bap == 0:
                            n["dither"] += 1
                            continue
                        if M.bad[r, k]:
                            n["bad"] += 1
                            continue
                        v = dequantised(int(M.codes[r, k]), bap, B.exp[r, k])
                        if r != A.CPL:
                            got = plane[0 if r == A.LFE else lfe + r, k]
                            assert got.view(np.uint32) == v.view(np.uint32), (seed, f, b, r, k, bap, int(M.codes[r, k]), got, v)
                            n["exact"] += 1
                            continue
                        bnd = sum(1 - x for x in strc[:(k - lo) // 12])                 # cplbndstrc 1: merged into the band below
                        for ch in range(nf):
                            if B.chincpl[ch]:
                                want = float(v) * co[ch][bnd]
                                got = float(plane[lfe + ch, k])
                                assert abs(got - want) <= 1e-6 * abs(want), (seed, f, b, ch, k, got, want)
                                n["coupled"] += 1
                n["cpl_blocks"] += A.CPL in B.rng
        L.orc_a52_free(st)
    print("acmod %d lfe %d: %d bins equal liba52's bit for bit, %d coupled values within 1e-6, %d bins with a code that is "
          "no level skipped, %d dither-only bins skipped; %d coupled blocks, %d with a short transform, %d with delta "
          "segments" % (acmod, lfe, n["exact"], n["coupled"], n["bad"], n["dither"], n["cpl_blocks"], n["short"], n["delta"]))
    assert n["exact"] > 4000 and n["short"] > 5 and n["delta"] > 5, n
    assert (n["coupled"] > 1000 and n["cpl_blocks"] > 5) == (acmod >= 2), n


# ---------------------------------------------------------------------------------------------------------------------
# the audit notices

def _one_frame():
    pcm = [H.gen_pcm(1, 6, seed=31, kind="music")]
    frames, t = _oracle(pcm, 6, 384000, 48000, H.CHMAP6)
    rows, shifts = MA.frame_rows(t["mdct"][0, 0], t["shift"][0, 0], 5, 1)
    P = A.parse_frame(frames[0, 0])
    return frames, [[rows]], [[shifts]], P, A.read_mantissas(frames[0, 0], P)


def _set_bits(frame, pos, width, value):
    bits = np.unpackbits(frame)
    bits[pos:pos + width] = [(value >> (width - 1 - i)) & 1 for i in range(width)]
    frame[:] = np.packbits(bits)


def test_audit_reports_a_flipped_bit():
    frames, rows, shifts, P, mant = _one_frame()
    hits = 0
    for blk, row, minbap in ((0, 0, 6), (3, 2, 6), (5, A.LFE, 6)):
        B, M = P.blocks[blk], mant[blk]
        k = int(np.nonzero(B.bap[row] >= minbap)[0][-1])           # an asymmetric field: every bit pattern is a level
        w = A.MANT_BITS[B.bap[row, k]]
        for bit in (0, w - 1):                                        # its first and its last bit
            damaged = frames.copy()
            _set_bits(damaged[0, 0], int(M.pos[row, k]) + bit, 1, 1 ^ int(M.codes[row, k]) >> (w - 1 - bit) & 1)
            rep = MA.Report()
            MA.audit_mantissas(rep, damaged, rows, shifts, "flip")
            assert rep.bins == [(0, 0, blk, row, k)] and len(rep.fails) == 1, rep.fails
            hits += 1
    assert hits == 6
    rep = MA.Report()
    MA.audit_mantissas(rep, frames, rows, shifts, "intact")
    rep.finish("the intact frame")


def test_audit_reports_two_swapped_fields():
    frames, rows, shifts, P, mant = _one_frame()
    B, M = P.blocks[2], mant[2]
    # two fields of the same width with different payloads, in different rows: one coding order off by a row would do this
    k0 = next(k for k in range(256) if B.bap[0, k] == 6)
    k1 = next(k for k in range(256) if B.bap[1, k] == 6 and M.codes[1, k] != M.codes[0, k0])
    damaged = frames.copy()
    _set_bits(damaged[0, 0], int(M.pos[0, k0]), 5, int(M.codes[1, k1]))
    _set_bits(damaged[0, 0], int(M.pos[1, k1]), 5, int(M.codes[0, k0]))
    rep = MA.Report()
    MA.audit_mantissas(rep, damaged, rows, shifts, "swap")
    assert rep.bins == [(0, 0, 2, 0, k0), (0, 0, 2, 1, k1)] and len(rep.fails) == 2, rep.fails


def test_audit_reports_stale_members_of_a_last_group():
    """a block whose last bap-1 group has unclaimed members: setting one is reported, and nothing else is"""
    frames, rows, shifts, P, mant = _one_frame()
    blk = next(b for b, M in enumerate(mant) if len(M.unused[1]) > 0)
    B, M = P.blocks[blk], mant[blk]
    r, k = max((int(M.pos[r, k]), r, k) for r in B.rng for k in range(256) if B.bap[r, k] == 1)[1:]
    g = int(np.unpackbits(frames[0, 0])[int(M.pos[r, k]):int(M.pos[r, k]) + 5].dot(1 << np.arange(4, -1, -1)))
    assert g % 3 == 0 and M.unused[1][-1] == 0
    damaged = frames.copy()
    _set_bits(damaged[0, 0], int(M.pos[r, k]), 5, g + 1)
    rep = MA.Report()
    MA.audit_mantissas(rep, damaged, rows, shifts, "stale")
    assert len(rep.fails) == 1 and rep.fails[0].startswith("unused | ") and not rep.bins, rep.fails
