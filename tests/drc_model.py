"""Numpy model of the encoder's dynamic range control (ac3mi_set_encode_drc, include/ac3mi.h): block energies, levels
relative to dialnorm, the five static curves, the per-stream smoothing, the dynrng codes and which blocks send them.
Exact integers throughout; the tables are built here in double precision from their definitions."""
import math

import numpy as np


def _lv(db):
    """dB -> lv (1/256 octave), round(256 dB / (20 log10 2))."""
    return int(round(256.0 * db / (20.0 * math.log10(2.0))))


LG = [int(round(256.0 * math.log2(1.0 + m / 256.0))) for m in range(256)]
XT = [int(round(32.0 * (2.0 ** (f / 256.0) - 1.0))) for f in range(256)]
DN = [_lv(d) for d in range(32)]

# profile -> (MB, Rb, N0, N1, C0, Re, Rc): boost limit, boost ratio, null band, early cut end, cut ratios
PROFILES = {
    1: (_lv(6), 2, 0, _lv(5), _lv(15), 2, 20),            # film standard
    2: (_lv(6), 2, _lv(-10), _lv(10), _lv(20), 2, 20),    # film light
    3: (_lv(12), 2, 0, _lv(5), _lv(15), 2, 20),           # music standard
    4: (_lv(12), 2, _lv(-10), _lv(10), _lv(10), 2, 2),    # music light
    5: (_lv(15), 5, 0, _lv(5), _lv(15), 2, 20),           # speech
}
ATTACK, RELEASE = 6631, 349


def lg(e):
    """256 floor(log2 e) + LG[8 fractional bits], e > 0."""
    k = int(e).bit_length() - 1
    m = ((int(e) << 8) >> k) & 255
    return 256 * k + LG[m]


def level(e):
    """A block's level L (lv) from its energy: about 0 for a full-scale sine on one channel, -4096 at most below."""
    return -4096 if e == 0 else max(-4096, lg(e) - 37 * 256)


def curve(r, profile):
    """The static gain g (lv) of `profile` at level r relative to dialogue."""
    mb, rb, n0, n1, c0, re, rc = PROFILES[profile]
    if r < n0:
        g = min(mb, ((n0 - r) * (rb - 1)) // rb)
    elif r <= n1:
        g = 0
    elif r <= c0:
        g = -(((r - n1) * (re - 1)) // re)
    else:
        g = -(((c0 - n1) * (re - 1)) // re) - (((r - c0) * (rc - 1)) // rc)
    return max(g, -1024)


def block_energies(pcm, chmap, nfbw):
    """pcm [F*1536][nch] s16 (input order), chmap (coded channel -> input channel) -> E [F][6], exact, over the coded
    full-bandwidth channels chmap[0 .. nfbw - 1]."""
    x = np.asarray(pcm, np.int64)
    F = x.shape[0] // 1536
    cols = [chmap[c] for c in range(nfbw)]
    sq = (x[:, cols] ** 2).sum(axis=1)
    return sq.reshape(F, 6, 256).sum(axis=2)


def step(s, g):
    """One block of smoothing: s moves toward g, attack when falling, release when rising, never past g."""
    d = g - s
    if d < 0:
        s -= max(1, (-d * ATTACK) >> 16)
    elif d > 0:
        s += max(1, (d * RELEASE) >> 16)
    return s


def code_of(s):
    """The dynrng value v (-128..127) of state s; the byte is v & 0xff."""
    return min(127, max(-128, 32 * (s >> 8) + XT[s & 255]))


def decoded_gain(v):
    """The gain liba52 applies for dynrng value v: (32 + X) 2^(Y - 5), X the low 5 bits, Y the signed top 3."""
    b = int(v) & 0xff
    y = (b >> 5) - 8 if b >= 128 else b >> 5
    return (32 + (b & 31)) * 2.0 ** (y - 5)


def sent(codes):
    """[F][6] codes -> [F][6] bool: block 0 always, block b > 0 when its code differs from block b - 1's."""
    c = np.asarray(codes)
    s = np.ones(c.shape, bool)
    s[:, 1:] = c[:, 1:] != c[:, :-1]
    return s


def gains(pcm, chmap, nfbw, profile, dialnorm):
    """[F][6] static gains (lv)."""
    e = block_energies(pcm, chmap, nfbw)
    return np.array([[curve(level(int(v)) + DN[dialnorm], profile) for v in row] for row in e], np.int64)


def encode(pcm, chmap, nfbw, profile, dialnorm=31, state=0):
    """One stream's PCM [F*1536][nch] -> (codes [F][6] as values -128..127, sent [F][6], final state, the states
    [F][6] after each block)."""
    g = gains(pcm, chmap, nfbw, profile, dialnorm)
    s = int(state)
    codes = np.zeros(g.shape, np.int64)
    states = np.zeros(g.shape, np.int64)
    for f in range(g.shape[0]):
        for b in range(6):
            s = step(s, int(g[f, b]))
            states[f, b] = s
            codes[f, b] = code_of(s)
    return codes, sent(codes), s, states
