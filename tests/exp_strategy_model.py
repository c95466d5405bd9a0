"""numpy model of the encoder's cost-based exponent strategies (ac3mi_set_encode_exp_strategy 1, the rule in include/ac3mi.h).

Exact integers throughout.  A row is described by its kind: "fbw" (a full-bandwidth channel of an uncoupled frame, range
[0, n)), "cplch" (a full-bandwidth channel of a coupled frame, [0, cplstrtmant)), "lfe" ([0, 7), D15 only) or "cpl" (the
coupling channel, [cs, ce)).  raw is [6][256], a channel's raw exponents per block.  Strategies: 1 = D15, 2 = D25, 3 = D45,
0 = reuse.  choose() is the dynamic programme the kernel runs, brute() the minimum over every sequence, ref_rule() mode 0's
rule; coded() the exponents a strategy sequence sends."""
import itertools

import numpy as np

from tests.bandwidth_model import _encode_exp, encode_exp

GS = {1: 1, 2: 2, 3: 4}


def groups(n, s):
    """Exponent groups of a channel coding bins [0, n) with strategy s (enc_syntax.h: syn_exp_groups; cpl_groups: syn_cpl_exp_groups)."""
    gs = GS[s]
    return (n + gs * 3 - 4) // (3 * gs)


def cpl_groups(cs, ce, s):
    return (ce - cs) // GS[s] // 3


def bits(kind, s, lo, hi):
    """Bits of one exponent set apart from the strategy field."""
    if kind == "cpl":
        return 4 + 7 * cpl_groups(lo, hi, s)
    g = groups(hi, s)
    return 4 + 7 * g + {"fbw": 8, "cplch": 2, "lfe": 0}[kind]


def strategies(kind):
    return (1,) if kind == "lfe" else (1, 2, 3)


def cpl_encode_exp(row, cs, ce, s):
    """The coupling channel's encode_exp (encode.hip cpl_encode_exp): entry i = min of bins cs + i gs .. + gs - 1, then
    min over j of g[j] + 2 |i - j|; returns the row with [cs, ce) replaced."""
    gs = GS[s]
    ne = (ce - cs) // gs
    g = np.array([int(np.min(row[cs + i * gs:cs + (i + 1) * gs])) for i in range(ne)], np.int64)
    i = np.arange(ne)
    c = (g[None, :] + 2 * np.abs(i[:, None] - i[None, :])).min(1)
    out = np.array(row, np.int64).copy()
    out[cs:ce] = np.repeat(c, gs)
    return out


def set_coded(kind, raw, i, L, s, lo, hi):
    """The coded exponents [lo, hi) of candidate set (i, L, s)."""
    raw = np.asarray(raw, np.int64)
    row = raw[i].copy()
    row[lo:hi] = raw[i:i + L, lo:hi].min(0)
    if kind == "cpl":
        return cpl_encode_exp(row, lo, hi, s)[lo:hi]
    return _encode_exp(row, hi, s)[lo:hi]


def cost(kind, raw, i, L, s, lo, hi):
    c = set_coded(kind, raw, i, L, s, lo, hi)
    r = np.asarray(raw, np.int64)[i:i + L, lo:hi]
    assert (c[None, :] <= r).all()
    return bits(kind, s, lo, hi) + int((r - c[None, :]).sum())


def seq_cost(kind, raw, strat, lo, hi):
    """J of a strategy sequence (block 0 must send)."""
    assert strat[0] != 0
    tot, b = 0, 0
    while b < 6:
        e = b + 1
        while e < 6 and strat[e] == 0:
            e += 1
        tot += cost(kind, raw, b, e - b, int(strat[b]), lo, hi)
        b = e
    return tot


_CHOSEN = {}


def choose(kind, raw, lo, hi):
    """The rule: -> (J(0), strategies [6]).  (Remembered per argument set: sweeps over one content ask the same rows again.)"""
    key = (kind, np.asarray(raw, np.int64).tobytes(), lo, hi)
    if key not in _CHOSEN:
        _CHOSEN[key] = _choose(kind, raw, lo, hi)
    return _CHOSEN[key][0], list(_CHOSEN[key][1])


def _choose(kind, raw, lo, hi):
    J = [0] * 7
    pick = [None] * 6
    for i in range(5, -1, -1):
        best = None
        for L in range(1, 7 - i):
            for s in strategies(kind):
                v = cost(kind, raw, i, L, s, lo, hi) + J[i + L]
                if best is None or v < best:
                    best, pick[i] = v, (L, s)
        J[i] = best
    st, i = [0] * 6, 0
    while i < 6:
        L, s = pick[i]
        st[i] = s
        i += L
    return J[0], st


def all_sequences(kind):
    for starts in itertools.product((0, 1), repeat=5):
        sb = [0] + [b + 1 for b in range(5) if starts[b]]
        for ss in itertools.product(strategies(kind), repeat=len(sb)):
            st = [0] * 6
            for b, s in zip(sb, ss):
                st[b] = s
            yield st


def brute(kind, raw, lo, hi):
    """-> (minimum J, [every sequence reaching it])."""
    best, arg = None, []
    for st in all_sequences(kind):
        v = seq_cost(kind, raw, st, lo, hi)
        if best is None or v < best:
            best, arg = v, [st]
        elif v == best:
            arg.append(st)
    return best, arg


def ref_rule(raw, lfe=False, lo=0, hi=256):
    """Mode 0's strategies (ENC/ac3enc.cpp:617-669): |differences| over bins [lo, hi) (256 bins for a channel, the coupling
    row is 24 outside its range), then the run length; the LFE only sends or reuses (D15)."""
    raw = np.asarray(raw, np.int64)
    st = [1] + [1 if int(np.abs(raw[b, lo:hi] - raw[b - 1, lo:hi]).sum()) > 1000 else 0 for b in range(1, 6)]
    if lfe:
        return st
    out = list(st)
    for b in range(6):
        if st[b]:
            run = 1
            while b + run < 6 and st[b + run] == 0:
                run += 1
            out[b] = 3 if run == 1 else 2 if run <= 3 else 1
    return out


def coded(kind, raw, strat, lo, hi):
    """[6][hi - lo] the exponents the frame sends on [lo, hi) under `strat` (a reuse block gets its run start's)."""
    if kind != "cpl":
        return encode_exp(raw, strat, hi)[:, lo:hi]
    raw = np.asarray(raw, np.int64)
    out = np.zeros((6, hi - lo), np.int64)
    b = 0
    while b < 6:
        e = b + 1
        while e < 6 and strat[e] == 0:
            e += 1
        out[b:e] = set_coded(kind, raw, b, e - b, int(strat[b]), lo, hi)
        b = e
    return out
