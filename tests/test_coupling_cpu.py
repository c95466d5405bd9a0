"""CPU: the coupling setter's declaration and export, and the numpy model of the rule (tests/coupling_model.py) on
hand-built rows."""
import os
from fractions import Fraction

import numpy as np

from tests import _harness as H
from tests import coupling_model as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_setter_declared_exported_and_bound():
    pkg = H.pkg()
    assert "ac3mi_set_encode_coupling" in pkg.declared_symbols()
    with open(os.path.join(ROOT, "include", "ac3mi.h")) as f:
        assert "int ac3mi_set_encode_coupling(ac3mi_ctx *ctx, int mode, int begf);" in f.read()
    lib = pkg.load_library()
    assert hasattr(lib, "ac3mi_set_encode_coupling")
    assert callable(getattr(pkg.Engine, "set_encode_coupling", None))


def _frame(nch, seed, shape=None):
    rng = np.random.default_rng(seed)
    base = rng.integers(-3000, 3000, (6, 256))
    rows = np.stack([base] * nch, 1) if shape is None else shape(base, rng)
    x = np.full((6, nch), 2, np.int64)
    return rows, x


def test_identical_channels_couple_with_equal_coordinates():
    for nfbw in (2, 3, 5):
        for begf in (0, 4, 12):
            rows, x = _frame(nfbw, 1)
            cplinu, mstr, codes = C.decide(rows, x, nfbw, begf)
            assert cplinu == 1
            assert len(set(mstr)) == 1 and all(c == codes[0] for c in codes)
            # identical rows: coordinate 2^g / nfbw (within the quantiser's step, never above)
            v = C.coord_value(codes[0][0], mstr[0])
            assert v <= (1 << C.cpl_g(nfbw)) / nfbw + 1e-12 and v > 0.9 * (1 << C.cpl_g(nfbw)) / nfbw


def test_antiphase_pair_is_not_coupled():
    rows, x = _frame(2, 2, lambda b, r: np.stack([b, -b], 1))
    assert C.decide(rows, x, 2, 0)[0] == 0


def test_switched_frames_are_not_coupled():
    rows, x = _frame(2, 3)
    assert C.decide(rows, x, 2, 0)[0] == 1
    assert C.decide(rows, x, 2, 0, switched=True)[0] == 0


def test_coupled_rematrixing_bands_end_at_cplstrtmant():
    assert C.remat_bands_coupled(0) == [(13, 25), (25, 37)]
    assert C.remat_bands_coupled(1) == [(13, 25), (25, 37), (37, 49)]
    assert C.remat_bands_coupled(2) == [(13, 25), (25, 37), (37, 61)]
    assert C.remat_bands_coupled(5) == [(13, 25), (25, 37), (37, 61), (61, 97)]
    # identical channels: every band flagged (S = 0); an independent channel 20 dB down: none
    rows, x = _frame(2, 7)
    assert C.remat_coupled(rows, x, 1) == [7] * 6
    rng = np.random.default_rng(8)
    rows = rng.integers(-3000, 3000, (6, 2, 256))
    rows[:, 1] //= 10
    assert C.remat_coupled(rows, x, 4) == [0] * 6
    assert C.remat_coupled(np.stack([rows[:, 0]] * 2, 1), x, 4, blksw=[[0, 1]] * 6) == [0] * 6


def test_silent_channel_gets_the_zero_coordinate():
    rows, x = _frame(2, 4, lambda b, r: np.stack([b, 0 * b], 1))
    cplinu, mstr, codes = C.decide(rows, x, 2, 2)
    assert cplinu == 1
    assert all(cd == 0xF0 for cd in codes[1])
    assert all(cd != 0xF0 for cd in codes[0])


def test_quantiser_is_the_largest_value_not_above_the_ratio():
    rng = np.random.default_rng(5)
    cases = [(0, 0), (0, 5), (5, 0), (1, 1), (1 << 40, 1), (1, 1 << 40), (3, 7)]
    cases += [(int(a), int(b)) for a, b in rng.integers(0, 1 << 45, (40, 2))]
    cases += [(int(a), int(a) * int(k)) for a, k in zip(rng.integers(1, 1 << 30, 20), rng.integers(1, 5000, 20))]
    for ech, ecpl in cases:
        for M in range(4):
            best = None
            for code in range(256):
                mant, s = C.coord(code, M)
                v = Fraction(mant, 1 << s)
                if v * v * ecpl <= ech and (best is None or v > best[0] or (v == best[0] and code < best[1])):
                    best = (v, code)
            got = C.quant(ech, ecpl, M)
            if ech == 0:                        # the zero coordinate, also at 0 / 0 where every value fits (include/ac3mi.h)
                assert got == 0xf0 and best[0] == (0 if ecpl else Fraction(31, 4) / 8 ** M), (ecpl, M, got, best)
                continue
            assert Fraction(*C.coord(got, M)[:1], 1 << C.coord(got, M)[1]) == best[0], (ech, ecpl, M, got, best)


def test_rematrix_band_sets_match_liba52():
    assert [C.remat_bands(b) for b in range(13)] == [2, 3, 3] + [4] * 10
    for begf in range(13):
        end = C.start_mant(begf)
        n = 0
        for top in C.REMAT_BAND_END:            # the bands liba52 reads: up to the first whose end reaches cplstrtmant
            n += 1
            if top >= end:
                break
        assert C.remat_bands(begf) == n


