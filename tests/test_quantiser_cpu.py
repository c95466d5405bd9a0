"""The packer's single-form mantissa quantiser (csrc/enc_mant.h: mant_quant_lut over the table entries mant_pack_entry builds)
against the encoder's two quantisers (ac3enc.cpp:1150-1190, restated in tests/quantiser_model.py as enc_mant.h documents them), in numpy and
without a GPU.  `quant_words` restates mant_pack_entry's arithmetic by hand: this pins the algebra, not the C table - a wrong
entry in mant_pack_entry is caught by the GPU parity tests (test_packer_quantiser_gpu.py, test_packer_golden_gpu.py,
test_encode_gpu.py), not here.

In contract - shift e in 0..23 and |c << e| < 2^24 - both quantisers are one expression over a four-word table entry:
  x = F * (Y mod 2^24) + (R_neg if Y < 0 else R_pos)   (mod 2^32, read as int32; Y = c << e)
  v = ((min(x, 2^29 - 1) << 2) mod 2^32) >> SH
This pins that algebra for every level count and every width, every e and a dense sweep of c including the edges."""
import numpy as np
import pytest

from tests.quantiser_model import ASYM_BITS, SYM_LEVELS, asym_quant, sym_quant


def quant_words(bap):
    """(F, R_pos, R_neg, SH) of a bap code, as mant_pack_entry / mant_pack_word compute them."""
    M = 1 << 32
    if bap == 0:
        return 0, 0, 0, 0
    if bap in SYM_LEVELS:
        L = SYM_LEVELS[bap]
        rp = (1 << 24) + ((L >> 1) << 25)
        return L, rp, (rp - (L << 24)) % M, 27
    w = ASYM_BITS[bap]
    rp = 1 << (29 - w)
    return 32, rp, (rp - (1 << 29)) % M, 32 - w


def quant_lut(c, e, words):
    """mant_quant_lut in 32-bit unsigned arithmetic."""
    F, rp, rn, sh = words
    M = 1 << 32
    Y = (c.astype(np.int64) << e)                               # |Y| < 2^24: no wrap
    r = np.where(Y < 0, rn, rp).astype(np.int64)
    x = (F * (Y % (1 << 24)) + r) % M                           # v_mad_u32_u24: the low 24 bits of Y
    x = np.where(x >= 1 << 31, x - M, x)                        # as int32
    x = np.minimum(x, (1 << 29) - 1)
    return ((x << 2) % M) >> sh


def c_sweep(e):
    lim = (1 << (24 - e)) - 1                                   # |c << e| < 2^24
    rng = np.random.default_rng(1000 + e)
    dense = np.arange(-min(lim, 4096), min(lim, 4096) + 1)
    edges = np.concatenate([lim - np.arange(min(lim, 64) + 1), -lim + np.arange(min(lim, 64) + 1)])
    # every rounding boundary of every quantiser lies on a multiple of 2^(s) or near one: sample around powers of two too
    p2 = np.array([(1 << k) + d for k in range(24 - e) for d in (-2, -1, 0, 1, 2)], dtype=np.int64)
    p2 = p2[np.abs(p2) <= lim]
    rand = rng.integers(-lim, lim + 1, size=20000)
    return np.unique(np.concatenate([dense, edges, p2, -p2, rand]).astype(np.int64))


@pytest.mark.parametrize("e", range(24))
def test_single_form_matches_both_quantisers(e):
    c = c_sweep(e)
    for bap, L in SYM_LEVELS.items():
        want = sym_quant(c, e, L)
        got = quant_lut(c, e, quant_words(bap))
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, "sym L=%d e=%d c=%d: %d != %d" % (L, e, c[bad[0]], got[bad[0]], want[bad[0]])
    for bap, w in ASYM_BITS.items():
        want = asym_quant(c, e, w)
        got = quant_lut(c, e, quant_words(bap))
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, "asym w=%d e=%d c=%d: %d != %d" % (w, e, c[bad[0]], got[bad[0]], want[bad[0]])


def test_bap0_is_zero():
    c = c_sweep(0)
    assert (quant_lut(c, 0, quant_words(0)) == 0).all()


def test_sym_never_reaches_the_clamp():
    # the clamp at 2^29 - 1 is the asymmetric quantiser's v >= m; a symmetric x stays below it
    for L in SYM_LEVELS.values():
        assert L * ((1 << 24) - 1) + (1 << 24) + ((L >> 1) << 25) < (1 << 29) - 1
