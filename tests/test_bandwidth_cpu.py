"""CPU: the bandwidth setter's declaration and export, and the numpy model of the rule (tests/bandwidth_model.py)."""
import os

import numpy as np

from tests import _harness as H
from tests import bandwidth_model as W
from tests import coupling_model as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the AC-3 bit rates in b/s (full rates; the half rates are these >> 1 and >> 2)
RATES = (32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384, 448, 512, 576, 640)


def test_setter_declared_exported_and_bound():
    pkg = H.pkg()
    assert "ac3mi_set_encode_bandwidth" in pkg.declared_symbols()
    with open(os.path.join(ROOT, "include", "ac3mi.h")) as f:
        assert "int ac3mi_set_encode_bandwidth(ac3mi_ctx *ctx, int mode, int chbwcod);" in f.read()
    lib = pkg.load_library()
    assert hasattr(lib, "ac3mi_set_encode_bandwidth")
    assert callable(getattr(pkg.Engine, "set_encode_bandwidth", None))


def test_band_arithmetic():
    assert [W.nbc(c) for c in (0, 13, 25, 32, 49, 50)] == [73, 112, 148, 169, 220, 223]
    assert [W.cplendf(c) for c in (0, 3, 4, 13, 32, 47, 48, 50)] == [0, 0, 1, 3, 8, 11, 12, 12]
    assert W.cplendmant(32) == 169 and W.cplendmant(50) == 217
    for c in range(51):
        assert 0 <= W.nbc(c) - W.cplendmant(c) <= 9
    assert W.cpl_bands(0, 50) == 15 and W.cpl_bands(2, 32) == 9 and W.cpl_bands(10, 32) == 1 and W.cpl_bands(11, 32) == 0
    assert W.remat_bands(148)[3] == (61, 148)


def test_mode2_spot_values():
    # the header's two examples
    assert W.mode2_chbwcod(48000, 96000, 2) == 25
    assert W.mode2_chbwcod(48000, 384000, 6) == 32
    # no cut from 96 kb/s per channel on
    assert W.mode2_chbwcod(48000, 192000, 2) == 50 and W.mode2_chbwcod(48000, 96000, 1) == 50
    assert W.mode2_chbwcod(48000, 640000, 6) == 50
    # 5.1 at 224 kb/s: 44 800 b/s a channel -> 11 kHz: (73 + 3c) 48000 <= 512 x 11000 -> c = 14
    assert W.mode2_chbwcod(48000, 224000, 6) == 14
    # 44.1 kHz and 32 kHz: the same cutoff spans more bins
    assert W.mode2_chbwcod(44100, 96000, 2) == 29          # 14 kHz: 512 x 14 000 / 44 100 = 162.5 bins -> c = 29
    assert W.mode2_chbwcod(44100, 384000, 6) == 37         # 16 kHz: 185.8 bins
    assert W.mode2_chbwcod(32000, 96000, 2) == 50          # 14 kHz at 32 kHz: 224 bins - everything
    assert W.mode2_chbwcod(32000, 64000, 2) == 34          # 32 000 b/s a channel -> 11 kHz: 176 bins
    # half rates: a 24 kHz stream at 48 kb/s stereo (24 000 b/s a channel -> 8 kHz: 170.7 bins -> c = 32)
    assert W.mode2_chbwcod(24000, 48000, 2) == 32
    assert W.mode2_chbwcod(22050, 48000, 2) == 37          # 8 kHz: 185.8 bins
    assert W.mode2_chbwcod(12000, 24000, 1) == 50          # 8 kHz at 12 kHz: beyond Nyquist - no cut


def test_mode2_is_monotone_in_rate():
    for sr in (48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000):
        half = 0 if sr >= 32000 else 1 if sr >= 16000 else 2
        for ch in range(1, 7):
            prev = -1
            for k in RATES:
                br = (k * 1000) >> half
                c = W.mode2_chbwcod(sr, br, ch)
                assert 0 <= c <= 50 and c >= prev, (sr, ch, br)
                if br // min(ch, 5) >= 96000:
                    assert c == 50
                prev = c


def test_encode_exp_invariants():
    """At every nbc the model's exponents keep the +-2 constraint, never exceed the raw minimum over the run, and the first
    is at most 15."""
    rng = np.random.default_rng(5)
    for strat in ([1, 0, 0, 0, 0, 0], [3, 2, 0, 1, 0, 0], [1, 1, 1, 1, 1, 1], [2, 0, 0, 3, 0, 0]):
        raw = rng.integers(0, 25, (6, 256))
        for n in (73, 112, 169, 220, 223):
            e = W.encode_exp(raw, strat, n)
            assert e.shape == (6, n)
            assert (e[:, 0] <= 15).all()
            b = 0
            while b < 6:
                end = b + 1
                while end < 6 and strat[end] == 0:
                    end += 1
                assert (e[b:end] == e[b]).all()
                assert (e[b, :n] <= raw[b:end, :n].min(0)).all()
                gs = {1: 1, 2: 2, 3: 4}[strat[b]]
                grp = e[b, 1::gs]
                assert (np.abs(np.diff(np.concatenate([[e[b, 0]], grp]))) <= 2).all()
                b = end


def test_coupling_end_follows_the_bandwidth():
    """Identical channels couple over cpl_bands(begf, c) bands; begf beyond cplendf + 2 never couples."""
    rng = np.random.default_rng(7)
    base = rng.integers(-3000, 3000, (6, 256))
    rows = np.stack([base] * 2, 1)
    x = np.full((6, 2), 2, np.int64)
    cplinu, mstr, codes = W.cpl_decide(rows, x, 2, 2, 32)
    assert cplinu == 1 and len(codes[0]) == 9 and codes[0] == codes[1]
    assert W.cpl_decide(rows, x, 2, 11, 32)[0] == 0
    assert len(W.cpl_decide(rows, x, 2, 0, 50)[2][0]) == 15


def test_coupling_at_chbwcod_50_is_the_coupling_rule():
    """At chbwcod 50 the restated decision is tests/coupling_model.py's, frame for frame."""
    rng = np.random.default_rng(9)
    for trial in range(12):
        nfbw = (2, 3, 5)[trial % 3]
        base = rng.integers(-4000, 4000, (6, 256))
        gains = rng.uniform(0.2, 1.0, nfbw)
        rows = np.stack([(base * gains[c]).astype(np.int64) + rng.integers(-300, 300, (6, 256)) * (trial % 2) for c in range(nfbw)], 1)
        if trial % 4 == 3:
            rows[:, 1] = -rows[:, 0]
        x = rng.integers(0, 4, (6, nfbw))
        for begf in (0, 5, 12):
            assert W.cpl_decide(rows, x, nfbw, begf, 50) == C.decide(rows, x, nfbw, begf)
