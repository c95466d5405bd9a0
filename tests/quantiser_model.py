"""The reference encoder's two mantissa quantisers (ac3enc.cpp:1150-1190) in numpy, as csrc/enc_mant.h documents them, and
what they make of a whole row: the model that tests/mantissa_audit.py holds every coded bin of an encoded frame against, and
that tests/test_quantiser_cpu.py holds the packer's single-form quantiser against.

The contract: a coefficient c is quantised at e = its encoded exponent - its block's shift.  In contract - c == 0, or e in
0..23 and |c| << e < 2^24 - the result is a property of (c, e, bap) alone.  Out of contract (a reuse run that pulls the
exponent of a strongly normalised block below its shift) the reference shifts by a negative count and writes what the x86
build makes of that; this model does not say what."""
import numpy as np

SYM_LEVELS = {1: 3, 2: 5, 3: 7, 4: 11, 5: 15}               # bap -> levels of the symmetric quantiser
ASYM_BITS = {b: b - 1 for b in range(6, 14)}
ASYM_BITS.update({14: 14, 15: 16})                            # bap -> width of the asymmetric quantiser


def sym_quant(c, e, levels):
    """ac3enc.cpp:1150-1166, 32-bit arithmetic (int64 here: in contract nothing wraps)."""
    c = c.astype(np.int64)
    a = np.abs(c) << e
    v = ((levels * a) >> 24) + 1 >> 1
    return np.where(c >= 0, (levels >> 1) + v, (levels >> 1) - v)


def asym_quant(c, e, qbits):
    """ac3enc.cpp:1169-1190; e a number or one per coefficient (e + qbits - 24 of either sign)."""
    c = c.astype(np.int64)
    lshift = np.asarray(e, np.int64) + qbits - 24
    v = np.where(lshift >= 0, c << np.maximum(lshift, 0), c >> np.maximum(-lshift, 0))
    v = (v + 1) >> 1
    m = 1 << (qbits - 1)
    v = np.minimum(v, m - 1)
    assert (v >= -m).all()
    return v & ((1 << qbits) - 1)


def in_contract(c, e):
    """where (c, e) is in the quantisers' contract: a zero coefficient at any e, else e in 0..23 and |c| << e < 2^24"""
    c, e = np.asarray(c, np.int64), np.asarray(e, np.int64)
    return (c == 0) | ((0 <= e) & (e <= 23) & (np.abs(c) << np.clip(e, 0, 23) < 1 << 24))


def expected_codes(c, e, bap):
    """The codes of a row: c, e, bap one per bin -> int64 per bin, -1 where bap is 0, -2 where the bin is out of contract.
    A zero coefficient gives the zero code at any e (levels >> 1 symmetric, 0 asymmetric)."""
    c, e, bap = np.asarray(c, np.int64), np.asarray(e, np.int64), np.asarray(bap, np.int64)
    ok = in_contract(c, e)
    c = np.where(ok, c, 0)
    e = np.where(c == 0, 0, e)
    out = np.full(c.shape, -1, np.int64)
    for b, levels in SYM_LEVELS.items():
        m = bap == b
        out[m] = sym_quant(c[m], e[m], levels)
    for b, w in ASYM_BITS.items():
        m = bap == b
        out[m] = asym_quant(c[m], e[m], w)
    out[~ok & (bap > 0)] = -2
    return out
