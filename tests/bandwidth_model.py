"""numpy model of the encoder's audio bandwidth (ac3mi_set_encode_bandwidth, the rule in include/ac3mi.h).

Exact integers throughout.  mode2_chbwcod() is the bit-rate table; nbc() / cplendf() / cpl_bands() the band arithmetic;
encode_exp() turns the mode-0 raw exponents and strategies (the encode taps d_exponent / d_exp_strategy, which do not
depend on the bandwidth) into the exponents the decoder sees on [0, nbc); remat_flags() and cpl_decide() are the
rematrixing and coupling decisions with the variable band ends, restated here on their own."""
import numpy as np

# (r >= threshold in b/s per full-bandwidth channel, cutoff Fc in Hz), first match wins; r >= 96 000: no cut
FC_TABLE = ((80000, 18000), (64000, 16000), (48000, 14000), (32000, 11000), (0, 8000))


def nbc(c):
    """Coded bins of a full-bandwidth channel for chbwcod c (liba52 parse.c:699: endmant = 73 + 3 chbwcod)."""
    return 73 + 3 * c


def mode2_chbwcod(sample_rate, bit_rate, channels):
    nfbw = min(channels, 5)
    r = bit_rate // nfbw
    if r >= 96000:
        return 50
    fc = next(f for t, f in FC_TABLE if r >= t)
    best = 0
    for c in range(51):
        if nbc(c) * sample_rate <= 512 * fc:
            best = c
    return best


def cplendf(c):
    return min(12, c >> 2)


def cplendmant(c):
    return 73 + 12 * cplendf(c)


def cpl_bands(begf, c):
    """Coupling bands of a coupled frame (3 + cplendf - begf); 0 or less: no frame couples."""
    return 3 + cplendf(c) - begf


def remat_bands(n):
    """Rematrixing bands of an uncoupled 2/0 frame coding n bins: the fourth ends at n (liba52 parse.c:840-864)."""
    return ((13, 25), (25, 37), (37, 61), (61, n))


def _encode_exp(exp, n, strategy):
    """The reference's encode_exp (ENC/ac3enc.cpp:684-761) on one row with nb_exps = n; bins it does not write keep exp's."""
    gs = {1: 1, 2: 2, 3: 4}[strategy]
    ng = ((n + gs * 3 - 4) // (3 * gs)) * 3
    e1 = [int(exp[0])] + [min(int(v) for v in exp[1 + i * gs:1 + (i + 1) * gs]) for i in range(ng)]
    e1[0] = min(e1[0], 15)
    while True:
        again = False
        for i in range(1, ng + 1):
            d = e1[i] - e1[i - 1]
            if d > 2:
                e1[i] = e1[i - 1] + 2
            elif d < -2:
                again = True
                e1[i - 1] = e1[i] + 2
        if not again:
            break
    out = np.array(exp, np.int64).copy()
    out[0] = e1[0]
    for i in range(ng):
        out[1 + i * gs:1 + (i + 1) * gs] = e1[i + 1]
    return out


def encode_exp(raw, strat, n):
    """raw [6][256] raw exponents of one channel, strat [6] its strategies (0 = reuse), n coded bins -> [6][n] the
    exponents sent (a reuse block gets its run start's): min over the run on [0, n), then encode_exp over nb_exps = n."""
    raw = np.asarray(raw, np.int64)
    out = np.zeros((6, n), np.int64)
    b = 0
    while b < 6:
        e = b + 1
        while e < 6 and strat[e] == 0:
            e += 1
        row = raw[b].copy()
        row[:n] = raw[b:e, :n].min(0)
        enc = _encode_exp(row, n, int(strat[b]))
        out[b:e] = enc[:n]
        b = e
    return out


def _ilog2(a):
    a = np.asarray(a, np.int64)
    return np.where(a > 0, np.frexp(np.maximum(a, 1).astype(np.float64))[1] - 1, 0)


def remat_flags(cl, cr, xl, xr, n):
    """One uncoupled 2/0 block: rows cl, cr [256] before exponents at exp_samples xl, xr (the mode-0 taps d_mdct /
    d_exp_samples) -> the flags: rows aligned to min(x), M = (L' + R') >> 1, S = (L' - R') >> 1, band flagged iff
    2 min(EM, ES) < min(EL, ER) over remat_bands(n)."""
    xm = min(int(xl), int(xr))
    a = np.asarray(cl, np.int64) >> (int(xl) - xm)
    b = np.asarray(cr, np.int64) >> (int(xr) - xm)
    m, s = (a + b) >> 1, (a - b) >> 1
    fl = 0
    for i, (lo, hi) in enumerate(remat_bands(n)):
        el, er = int((a[lo:hi] ** 2).sum()), int((b[lo:hi] ** 2).sum())
        em, es = int((m[lo:hi] ** 2).sum()), int((s[lo:hi] ** 2).sum())
        if 2 * min(em, es) < min(el, er):
            fl |= 1 << i
    return fl


def _cpl_g(nfbw):
    return 1 if nfbw <= 2 else 2 if nfbw <= 4 else 3


def _coord(code, M):
    E, m = code >> 4, code & 15
    return (16 + m, E + 3 * M + 2) if E < 15 else (m, 16 + 3 * M)


def _quant(ech, ecpl, M):
    if ech == 0:                            # the zero coordinate, also where Ecpl = 0 lets every value fit
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


def cpl_decide(rows, x, nfbw, begf, c, switched=False):
    """One frame: rows [6][nch][256], x [6][nch] (mode-0 taps) -> (cplinu, mstrcplco [nfbw], codes [nfbw][nb]) with the
    coupling range [37 + 12 begf, cplendmant(c)) in cpl_bands(begf, c) bands of 12 (ac3mi_set_encode_coupling's rule)."""
    cs, ce, nb, g = 37 + 12 * begf, cplendmant(c), cpl_bands(begf, c), _cpl_g(nfbw)
    if switched or nb <= 0:
        return 0, None, None
    xf = min(int(x[b][ch]) for b in range(6) for ch in range(nfbw))
    ech = [[0] * nb for _ in range(nfbw)]
    ecpl = [0] * nb
    for b in range(6):
        xb = min(int(x[b][ch]) for ch in range(nfbw))
        s = np.zeros(256, np.int64)
        for ch in range(nfbw):
            s += np.asarray(rows[b][ch], np.int64) >> (int(x[b][ch]) - xb)
            a = np.asarray(rows[b][ch][cs:ce], np.int64) >> (int(x[b][ch]) - xf)
            sq = (a * a).reshape(nb, 12).sum(1)
            for k in range(nb):
                ech[ch][k] += int(sq[k])
        v = s[cs:ce] >> g
        e = np.where(v != 0, 23 - _ilog2(np.abs(v)) + xb, 24)
        v = np.where(e >= 24, 0, v)
        q = v >> (xb - xf)
        sq = (q * q).reshape(nb, 12).sum(1)
        for k in range(nb):
            ecpl[k] += int(sq[k])
    for k in range(nb):
        if ecpl[k] << (2 * g + 2) < sum(ech[ch][k] for ch in range(nfbw)):
            return 0, None, None
    mstr, codes = [], []
    for ch in range(nfbw):
        best, bscore, bcodes = 0, -1, None
        for M in range(4):
            cc = [_quant(ech[ch][k], ecpl[k], M) for k in range(nb)]
            score = 0
            for cd in cc:
                mant, s_ = _coord(cd, M)
                score += (mant * mant) << (50 - 2 * s_)
            if score > bscore:
                best, bscore, bcodes = M, score, cc
        mstr.append(best)
        codes.append(bcodes)
    return 1, mstr, codes
