"""CPU: the exponent-strategy setter's declaration and export, and the numpy model of the cost rule
(tests/exp_strategy_model.py): the dynamic programme against brute force, against the reference's rule, and the reference's
rule and exponent coding against the oracle encoder."""
import ctypes
import os

import numpy as np
import pytest

from tests import _harness as H
from tests import exp_strategy_model as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_setter_declared_exported_and_bound():
    pkg = H.pkg()
    assert "ac3mi_set_encode_exp_strategy" in pkg.declared_symbols()
    with open(os.path.join(ROOT, "include", "ac3mi.h")) as f:
        assert "int ac3mi_set_encode_exp_strategy(ac3mi_ctx *ctx, int mode);" in f.read()
    lib = pkg.load_library()
    assert hasattr(lib, "ac3mi_set_encode_exp_strategy")
    assert callable(getattr(pkg.Engine, "set_encode_exp_strategy", None))


def _packer_groups(n, s):
    """enc_syntax.h syn_exp_groups (encode_exp_wave_t codes three entries a group)."""
    gs = {1: 1, 2: 2, 3: 4}[s]
    return ((n + gs * 3 - 4) // (3 * gs)) * 3 // 3


def test_group_counts():
    for n in range(73, 224):
        for s in (1, 2, 3):
            assert X.groups(n, s) == _packer_groups(n, s), (n, s)
    assert [X.groups(223, s) for s in (1, 2, 3)] == [74, 37, 19]
    assert X.groups(7, 1) == 2 and X.bits("lfe", 1, 0, 7) == 18
    for begf in range(13):
        cs = 37 + 12 * begf
        for endf in range(max(0, begf - 2), 13):
            ce = 73 + 12 * endf
            for s in (1, 2, 3):
                gs = {1: 1, 2: 2, 3: 4}[s]
                assert X.cpl_groups(cs, ce, s) == ((ce - cs) // gs) // 3       # enc_syntax.h syn_cpl_exp_groups
    assert X.bits("fbw", 1, 0, 223) == 4 + 7 * 74 + 8 and X.bits("cplch", 3, 0, 37) == 4 + 7 * 3 + 2
    assert X.bits("cpl", 2, 37, 217) == 4 + 7 * 30


def _rows(rng, kind):
    """Random and crafted raw rows [6][256] (values 0..24)."""
    if kind == "random":
        return rng.integers(0, 25, (6, 256))
    if kind == "smooth":
        base = np.clip(np.cumsum(rng.integers(-1, 2, 256)) // 4 + 12, 0, 24)
        return np.stack([np.clip(base + rng.integers(-1, 2, 256), 0, 24) for _ in range(6)])
    if kind == "steps":
        out = np.zeros((6, 256), np.int64)
        for b in range(6):
            out[b] = np.clip(5 + 3 * b * (rng.integers(0, 2)) + np.arange(256) // 40, 0, 24)
        return out
    if kind == "transient":
        out = np.tile(np.clip(np.arange(256) // 12 + 4, 0, 24), (6, 1))
        out[int(rng.integers(0, 6))] -= 4
        return np.clip(out, 0, 24)
    return np.full((6, 256), int(rng.integers(0, 25)))


ROWS = [("fbw", 0, 223), ("fbw", 0, 148), ("fbw", 0, 73), ("fbw", 0, 190), ("cplch", 0, 37), ("cplch", 0, 109),
        ("lfe", 0, 7), ("cpl", 37, 217), ("cpl", 61, 169), ("cpl", 133, 217)]


@pytest.mark.parametrize("kind,lo,hi", ROWS)
def test_dp_is_the_brute_force_minimum(kind, lo, hi):
    rng = np.random.default_rng(1000 * hi + lo + len(kind))
    n_seq = sum(1 for _ in X.all_sequences(kind))
    assert n_seq == (32 if kind == "lfe" else 3072)
    for content in ("random", "smooth", "steps", "transient", "flat"):
        raw = _rows(rng, content)
        if kind == "cpl":
            raw[:, :lo] = 24
            raw[:, hi:] = 24
        J, st = X.choose(kind, raw, lo, hi)
        best, args = X.brute(kind, raw, lo, hi)
        assert J == best, (content, J, best)
        assert X.seq_cost(kind, raw, st, lo, hi) == J
        if len(args) == 1:
            assert st == args[0], (content, st, args)
        assert J <= X.seq_cost(kind, raw, X.ref_rule(raw, kind == "lfe"), lo, hi)


def _oracle_encode(pcm, nch, rate):
    L = H.orc()
    fb = H.ci()
    h = L.orc_ac3enc_init(48000, rate, nch, ctypes.byref(fb))
    assert h
    cm = (ctypes.c_uint8 * 8)(*(list(H.CHMAP6 if nch == 6 else range(nch)) + [0] * 8)[:8])
    F = pcm.shape[0] // 1536
    out = []
    pcm = np.ascontiguousarray(pcm)
    for f in range(F):
        fr = np.zeros(fb.value, np.uint8)
        assert L.orc_ac3enc_frame(h, H.P(fr, H.u8p), ctypes.cast(pcm.ctypes.data + f * 1536 * nch * 2, H.i16p), cm) == fb.value
        m = np.zeros((6, 6, 256), np.int32)
        e1, e2 = np.zeros((6, 6, 256), np.uint8), np.zeros((6, 6, 256), np.uint8)
        st, sh = np.zeros((6, 6), np.uint8), np.zeros((6, 6), np.int8)
        c, fs = H.ci(), H.ci()
        L.orc_ac3enc_get_mdct(h, H.P(m, H.i32p))
        L.orc_ac3enc_get_exp(h, H.P(e1, H.u8p), H.P(e2, H.u8p))
        L.orc_ac3enc_get_misc(h, H.P(st, H.u8p), H.P(sh, H.i8p), ctypes.byref(c), ctypes.byref(fs))
        # (the exponent tap holds run starts after the min-merge: the raw exponents come from the rows and exp_samples)
        a = np.abs(m.astype(np.int64))
        lg = np.where(a > 0, np.frexp(np.maximum(a, 1).astype(np.float64))[1] - 1, 0)
        raw = np.where(a > 0, np.minimum(23 - lg + sh[..., None].astype(np.int64), 24), 24)
        out.append((raw, e2.copy(), st.copy()))
    L.orc_ac3enc_free(h)
    return out


@pytest.mark.parametrize("nch,rate,kind", [(6, 384000, "music"), (2, 192000, "tones"), (1, 96000, "music")])
def test_reference_rule_and_coding_against_the_oracle(nch, rate, kind):
    """On harness content the model's reference rule gives the oracle's strategies and its coding the oracle's exponents;
    the cost rule's J is never above the reference rule's."""
    pcm = H.gen_pcm(3, nch, seed=17, kind=kind)
    lfe = nch == 6
    for raw, enc, st in _oracle_encode(pcm, nch, rate):
        for ch in range(nch):
            is_lfe = lfe and ch == nch - 1
            rows = raw[:, ch].astype(np.int64)
            want = [int(v) for v in st[:, ch]]
            assert X.ref_rule(rows, is_lfe) == want, (ch, want)
            n = 7 if is_lfe else 223
            k = "lfe" if is_lfe else "fbw"
            assert np.array_equal(X.coded(k, rows, want, 0, n), enc[:, ch, :n].astype(np.int64)), ch
            J, _ = X.choose(k, rows, 0, n)
            assert J <= X.seq_cost(k, rows, want, 0, n)
