"""numpy model of the encoder's stereo rematrixing (ac3mi_set_encode_rematrix 1, the definition in include/ac3mi.h).

block_v() derives each channel-block's block-floating-point exponent v from the PCM, as enc_mdct_kernel does before its
transform; rematrix() takes the rows the kernel holds before exponents (the mode-0 MDCT tap: equal to them wherever
v <= 9, i.e. wherever a block's largest windowed sample is 32 or more) and returns the mode-1 rows, the band flags and
rematstr of every block."""
import ctypes

import numpy as np

BANDS = ((13, 25), (25, 37), (37, 61), (61, 223))

_WIN = None


def window():
    """The encoder's 256-entry half window (ac3mi_encode_spec_tables)."""
    global _WIN
    if _WIN is None:
        from tests import _harness as H
        lib = H.pkg().load_library()
        w = np.zeros(256, np.int16)
        lib.ac3mi_encode_spec_tables.restype = ctypes.c_int
        lib.ac3mi_encode_spec_tables(w.ctypes.data_as(ctypes.c_void_p), *([None] * 12))
        _WIN = w
    return _WIN


def _ilog2(a):
    """floor(log2(a)) for a > 0 (exact below 2^53: frexp's exponent), 0 for a = 0."""
    a = np.asarray(a, np.int64)
    return np.where(a > 0, np.frexp(a.astype(np.float64))[1] - 1, 0).astype(np.int64)


def block_v(pcm, chmap, last=None, win=None):
    """pcm [F*1536][nch] s16 (input order), last [nch][256] (coded order) or None -> v [F][6][nch]: (x * w) >> 15 over the
    block's 512 samples (the 256 before || the 256 new), v = 14 - ilog2(max |.|) clamped at 0, ilog2(0) = 0."""
    w = window() if win is None else np.asarray(win)
    w512 = np.concatenate([w, w[::-1]]).astype(np.int64)
    F = pcm.shape[0] // 1536
    nch = len(chmap)
    v = np.zeros((F, 6, nch), np.int64)
    for ch in range(nch):
        h = np.zeros(256, np.int64) if last is None else np.asarray(last[ch], np.int64)
        x = np.concatenate([h, pcm[:, chmap[ch]].astype(np.int64)])
        z = np.lib.stride_tricks.sliding_window_view(x, 512)[::256][:F * 6]
        m = np.abs((z * w512) >> 15).max(-1)
        v[:, :, ch] = np.maximum(14 - _ilog2(m), 0).reshape(F, 6)
    return v


def decide(cl, cr, vl, vr):
    """One block: rows cl, cr [256], exponents vl, vr -> (flags bit set, L', R', M, S)."""
    vm = min(vl, vr)
    a = np.asarray(cl, np.int64) >> (vl - vm)
    b = np.asarray(cr, np.int64) >> (vr - vm)
    m = (a + b) >> 1
    s = (a - b) >> 1
    flags = 0
    for i, (lo, hi) in enumerate(BANDS):
        el, er = int((a[lo:hi] ** 2).sum()), int((b[lo:hi] ** 2).sum())
        em, es = int((m[lo:hi] ** 2).sum()), int((s[lo:hi] ** 2).sum())
        if 2 * min(em, es) < min(el, er):
            flags |= 1 << i
    return flags, a, b, m, s


def rematrix(rows, v, blksw=None):
    """rows [F][6][2][256] (pre-exponent), v [F][6][2], blksw [F][6][2] or None
    -> (rows [F][6][2][256] as coded, shift [F][6][2] = v - 9 as coded, flags [F][6], rematstr [F][6])."""
    rows = np.asarray(rows, np.int64)
    F = rows.shape[0]
    out = rows.copy()
    shift = np.asarray(v, np.int64) - 9
    flags = np.zeros((F, 6), np.int64)
    rematstr = np.zeros((F, 6), np.int64)
    for f in range(F):
        prev = 0
        for b in range(6):
            vl, vr = int(v[f, b, 0]), int(v[f, b, 1])
            fl, a, r, m, s = decide(rows[f, b, 0], rows[f, b, 1], vl, vr)
            if blksw is not None and blksw[f, b, 0] != blksw[f, b, 1]:
                fl = 0
            if fl:
                lrow, rrow = a.copy(), r.copy()
                for i, (lo, hi) in enumerate(BANDS):
                    if (fl >> i) & 1:
                        lrow[lo:hi] = m[lo:hi]
                        rrow[lo:hi] = s[lo:hi]
                sh = min(vl, vr) - 9
                for c, row in ((0, lrow), (1, rrow)):
                    if sh > 0:              # the exponent stage codes |c| < 2^shift as exponent 24, value 0
                        row = np.where(np.abs(row) < (1 << sh), 0, row)
                    out[f, b, c] = row
                    shift[f, b, c] = sh
            flags[f, b] = fl
            rematstr[f, b] = 1 if b == 0 or fl != prev else 0
            prev = fl
    return out, shift, flags, rematstr
