"""numpy model of the encoder's channel coupling (ac3mi_set_encode_coupling 1, the rule in include/ac3mi.h).

decide() takes the channels' rows and exp_samples as the mode-0 encode taps give them (d_mdct, d_exp_samples) and returns
the frame decisions, mstrcplco and the coordinate codes.  Integer arithmetic only (Python ints where a product can pass
64 bits), so the model is exact."""
import numpy as np

REMAT_BAND_END = (25, 37, 61, 253)          # liba52 parse.c:669-678 (rematrix_band)


def cpl_g(nfbw):
    return 1 if nfbw <= 2 else 2 if nfbw <= 4 else 3


def start_mant(begf):
    return 37 + 12 * begf


def nbands(begf):
    return 15 - begf


def coord(code, M):
    """(mant, s) of coordinate code E << 4 | m under mstrcplco M: value mant * 2^-s (liba52 parse.c:642-656, x8 included)."""
    E, m = code >> 4, code & 15
    return (16 + m, E + 3 * M + 2) if E < 15 else (m, 16 + 3 * M)


def coord_value(code, M):
    mant, s = coord(code, M)
    return mant / float(1 << s)


def quant(ech, ecpl, M):
    """The largest coordinate value v (code) with v^2 Ecpl <= Ech, exactly; Ech = 0 gives the zero coordinate (E 15, m 0),
    with Ecpl = 0 as well (a band of digital silence, where every value fits)."""
    ech, ecpl = int(ech), int(ecpl)
    if ech == 0:
        return 15 << 4
    for E in range(15):
        s = E + 3 * M + 2
        if 256 * ecpl <= ech << (2 * s):
            m = 15
            while (16 + m) ** 2 * ecpl > ech << (2 * s):
                m -= 1
            return E << 4 | m
    s = 16 + 3 * M
    m = 15
    while m > 0 and m * m * ecpl > ech << (2 * s):
        m -= 1
    return 15 << 4 | m


def remat_bands(begf):
    """Rematrixing flags a coupled 2/0 block 0 sends: liba52's do ... while (rematrix_band[i++] < cplstrtmant)."""
    end, i = start_mant(begf), 0
    while True:
        i += 1
        if REMAT_BAND_END[i - 1] >= end:
            return i


def coupling_rows(rows, x, nfbw, begf):
    """rows [6][nch][256], x [6][nch] -> the coupling rows [6][256] (after the exponent cut) and their exp_samples [6]."""
    cs, g = start_mant(begf), cpl_g(nfbw)
    out = np.zeros((6, 256), np.int64)
    xb = np.zeros(6, np.int64)
    for b in range(6):
        xb[b] = min(int(x[b][c]) for c in range(nfbw))
        s = np.zeros(256, np.int64)
        for c in range(nfbw):
            s += np.asarray(rows[b][c], np.int64) >> (int(x[b][c]) - xb[b])
        v = np.zeros(256, np.int64)
        v[cs:217] = s[cs:217] >> g
        a = np.abs(v)
        lg = np.where(a > 0, np.frexp(np.maximum(a, 1).astype(np.float64))[1] - 1, 0)
        e = np.where(a > 0, 23 - lg + xb[b], 24)
        v[e >= 24] = 0
        out[b] = v
    return out, xb


def energies(rows, x, nfbw, begf):
    """-> Ech [nfbw][nb], Ecpl [nb] as Python ints."""
    cs, nb = start_mant(begf), nbands(begf)
    cpl, xb = coupling_rows(rows, x, nfbw, begf)
    xf = min(int(x[b][c]) for b in range(6) for c in range(nfbw))
    ech = [[0] * nb for _ in range(nfbw)]
    ecpl = [0] * nb
    for b in range(6):
        for c in range(nfbw):
            a = np.asarray(rows[b][c][cs:217], np.int64) >> (int(x[b][c]) - xf)
            sq = (a * a).reshape(nb, 12).sum(1)
            for k in range(nb):
                ech[c][k] += int(sq[k])
        q = cpl[b][cs:217] >> (int(xb[b]) - xf)
        sq = (q * q).reshape(nb, 12).sum(1)
        for k in range(nb):
            ecpl[k] += int(sq[k])
    return ech, ecpl


def decide(rows, x, nfbw, begf, switched=False):
    """One frame: rows [6][nch][256], x [6][nch] (mode-0 taps) -> (cplinu, mstrcplco [nfbw], codes [nfbw][nb])."""
    nb, g = nbands(begf), cpl_g(nfbw)
    if switched:
        return 0, None, None
    ech, ecpl = energies(rows, x, nfbw, begf)
    for k in range(nb):
        if ecpl[k] << (2 * g + 2) < sum(ech[c][k] for c in range(nfbw)):
            return 0, None, None
    mstr, codes = [], []
    for c in range(nfbw):
        best, bscore, bcodes = 0, -1, None
        for M in range(4):
            cc = [quant(ech[c][k], ecpl[k], M) for k in range(nb)]
            score = 0
            for cd in cc:
                mant, s = coord(cd, M)
                score += (mant * mant) << (50 - 2 * s)
            if score > bscore:
                best, bscore, bcodes = M, score, cc
        mstr.append(best)
        codes.append(bcodes)
    return 1, mstr, codes


def remat_bands_coupled(begf):
    """The rematrixing bands of a coupled 2/0 block: liba52's first remat_bands(begf) bands, the last ending at cplstrtmant."""
    edges = (13, 25, 37, 61)
    n = remat_bands(begf)
    return [(edges[i], edges[i + 1] if i + 1 < n else start_mant(begf)) for i in range(n)]


def remat_coupled(rows, x, begf, blksw=None):
    """A coupled 2/0 frame with rematrixing on: rows [6][2][256], x [6][2] (the rows before rematrixing), blksw [6][2] or
    None -> the flags of each block (the mode-1 rule of ac3mi_set_encode_rematrix over remat_bands_coupled(begf))."""
    flags = []
    for b in range(6):
        fl = 0
        if blksw is None or blksw[b][0] == blksw[b][1]:
            vl, vr = int(x[b][0]), int(x[b][1])
            vm = min(vl, vr)
            a = np.asarray(rows[b][0], np.int64) >> (vl - vm)
            c = np.asarray(rows[b][1], np.int64) >> (vr - vm)
            m, s = (a + c) >> 1, (a - c) >> 1
            for i, (lo, hi) in enumerate(remat_bands_coupled(begf)):
                el, er = int((a[lo:hi] ** 2).sum()), int((c[lo:hi] ** 2).sum())
                em, es = int((m[lo:hi] ** 2).sum()), int((s[lo:hi] ** 2).sum())
                if 2 * min(em, es) < min(el, er):
                    fl |= 1 << i
        flags.append(fl)
    return flags
