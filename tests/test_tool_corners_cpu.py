"""CPU: the level corners (tests/_tools.corner_batch: digital silence, full-scale squares with -32768, single full-scale
samples, full-scale DC, full-scale noise, the same square in every channel, the square with its rails swapped between
channels, silence into full scale in mid-frame) are well-posed content for the encoder tools, before
tests/test_tool_corners_gpu.py judges a kernel on them.

* the reference encoder (the oracle, pinned byte for byte to ac3enc) codes every frame of them at both rates of the budget
  matrix, and the mantissa audit of its frames against its own stage arrays leaves no bin out: whatever a tool's frames
  leave out of the quantisers' contract is the tool's doing, and the 1 % cap of tests/test_tool_mantissas_gpu.py applies;
* the numpy models of block switching, coupling, rematrixing and DRC run on them without a floating-point exception or a
  warning (they are exact integer models: a kernel that wraps, saturates or divides differently shows as a mismatch, but
  only if the model itself stays exact there), and their decisions are pinned as literals - they say which paths the GPU
  file reaches: zero energies quantised to coordinates (silence couples), rails that cancel (antiphase never couples,
  rematrixes everywhere), a DRC word in every block down to code -112."""
import warnings

import numpy as np
import pytest

from tests import _harness as H
from tests import _tools as T
from tests import bandwidth_model as W
from tests import block_switch_model as B
from tests import coupling_model as C
from tests import drc_model as D
from tests import mantissa_audit as MA
from tests import rematrix_model as R
from tests.test_encode_gpu import _oracle
from tests.test_frame_budget_gpu import RATES
from tests.test_mantissa_reader_cpu import oracle_audit

F = 3
FULL_SCALE = ("rails", "dc", "noise", "rails_identical", "rails_antiphase")

# cplinu of frames 0..2 by (kind, channels, begf); one entry where channels or begf do not matter
ALL, NONE, LATE = [1, 1, 1], [0, 0, 0], [0, 1, 1]
COUPLES = {"silence": ALL, "impulses": ALL, "noise": ALL, "rails_identical": ALL, "onset": ALL, "rails_antiphase": NONE, "dc": LATE,
           ("rails", 2, 0): LATE, ("rails", 2, 7): ALL, ("rails", 6, 0): ALL, ("rails", 6, 7): ALL}
# blksw summed over the stream, 2 / 6 channels (2 / 5 full-bandwidth channels): one switched block a channel wherever
# full scale begins against silence (the zero history in block 0; `onset`: block 2 of frame 1)
BLKSW = {"silence": (0, 0), "impulses": (31, 72), "rails": (2, 5), "dc": (2, 5), "noise": (2, 5), "rails_identical": (2, 5),
         "rails_antiphase": (2, 5), "onset": (2, 5)}
# profile 1 at dialnorm 24: (dynrng words sent of 18 blocks, lowest and highest code), 2 / 6 channels
DRC = {"silence": ((5, 0, 2),) * 2, "impulses": ((5, 0, 2),) * 2, "rails": ((18, -112, -16),) * 2, "dc": ((18, -112, -16),) * 2,
       "rails_identical": ((18, -112, -16),) * 2, "rails_antiphase": ((18, -112, -16),) * 2,
       "noise": ((18, -65, -10), (18, -100, -14)), "onset": ((13, -84, 1), (13, -85, 1))}
# rematrixing flag words [frame][block] (band 0 in bit 0) of the 2/0 streams whose flags do not depend on a seed
REMAT = {"silence": [[0] * 6] * 3, "rails_identical": [[15] * 6] * 3, "dc": [[15, 3, 3, 3, 3, 3]] + [[3] * 6] * 2,
         "rails_antiphase": [[15, 15, 13, 15, 15, 15], [15, 13, 15, 15, 15, 15], [13, 15, 15, 15, 15, 13]],
         "onset": [[0] * 6, [0, 0, 15, 15, 15, 15], [15] * 6],
         "rails": [[0, 3, 1, 3, 1, 3], [3, 1, 3, 1, 3, 3], [1, 3, 1, 3, 3, 1]]}


@pytest.fixture(scope="module")
def strict():
    with np.errstate(all="raise"), warnings.catch_warnings():
        warnings.simplefilter("error")
        yield


def test_the_content_is_what_it_says():
    for nch in (1, 2, 6):
        x = T.corner_batch(nch)
        assert x.shape == (8, F * 1536, nch) and x.dtype == np.int16
        k = {n: x[i].astype(np.int64) for i, n in enumerate(T.CORNER_KINDS)}
        assert not k["silence"].any() and set(np.unique(k["rails"])) == {-32768, 32767} == set(np.unique(k["rails_identical"]))
        assert (k["rails_identical"] == k["rails_identical"][:, :1]).all()
        assert not k["onset"][:1536 + 700].any() and np.array_equal(k["onset"][1536 + 700:], k["rails_identical"][1536 + 700:])
        assert np.abs(k["impulses"]).max() >= 32767 and (k["impulses"] != 0).mean() < 0.01
        assert set(np.unique(k["dc"])) <= {-32768, 32767} and (k["dc"] == k["dc"][:1]).all()
        if nch > 1:
            assert ((k["rails_antiphase"][:, 0] + k["rails_antiphase"][:, 1]) == -1).all()
        assert np.array_equal(T.corner("noise", nch, F, 904), H.gen_pcm(F, nch, seed=904, kind="noise"))


@pytest.mark.parametrize("hi", [0, 1])
@pytest.mark.parametrize("nch", [1, 2, 6])
def test_the_reference_encoder_leaves_no_bin_out(nch, hi):
    rep = MA.Report()
    oracle_audit(rep, list(T.corner_batch(nch)), nch, RATES[nch][hi], 48000, "corners %d ch" % nch)
    rep.finish("oracle on the level corners, %d channels at %d b/s" % (nch, RATES[nch][hi]))
    assert rep.n["frames"] == 8 * F and rep.n["compared"] > 0 and rep.n["left_out"] == 0, rep.n


@pytest.fixture(scope="module")
def stages():
    """channels -> (pcm [8][F*1536][nch], the oracle's mdct and shift arrays [8][F][6][6]...) at the higher matrix rate"""
    out = {}
    for nch in (2, 6):
        pcm = T.corner_batch(nch)
        _, t = _oracle(list(pcm), nch, RATES[nch][1], 48000, H.CHMAP6 if nch == 6 else tuple(range(8)))
        out[nch] = (pcm, t["mdct"], t["shift"])
    return out


@pytest.mark.parametrize("begf", [0, 7])
@pytest.mark.parametrize("nch", [2, 6])
def test_coupling_decisions(strict, stages, nch, begf):
    pcm, mdct, shift = stages[nch]
    nfbw = min(nch, 5)
    for i, kind in enumerate(T.CORNER_KINDS):
        want = COUPLES.get(kind, COUPLES.get((kind, nch, begf)))
        got = [C.decide(mdct[i, f], shift[i, f], nfbw, begf) for f in range(F)]
        assert [g[0] for g in got] == want, (kind, [g[0] for g in got])
        for cplinu, mstr, codes in got:
            if cplinu:                      # a decision comes with side information a frame can carry
                assert len(mstr) == nfbw and all(0 <= m <= 3 for m in mstr)
                assert all(len(c) == C.nbands(begf) and all(0 <= v <= 255 for v in c) for c in codes)
    # digital silence: every band energy is zero, and the frame couples - the kernel quantises coordinates from zero energies.
    # Every value satisfies v^2 Ecpl <= Ech there; the rule gives the zero coordinate (the largest one would play the
    # decoder's dither of the coupling channel 7.75 times louder than mode 0 leaves it)
    ech, ecpl = C.energies(mdct[0, 0], shift[0, 0], nfbw, begf)
    assert not any(ecpl) and not any(any(e) for e in ech)
    _, mstr, codes = C.decide(mdct[0, 0], shift[0, 0], nfbw, begf)
    assert mstr == [0] * nfbw and all(cd == 0xf0 for c in codes for cd in c)
    assert C.coord_value(0xf0, 0) == 0.0 and W.cpl_decide(mdct[0, 0], shift[0, 0], nfbw, begf, 50) == (1, mstr, codes)
    # the rows of the full-scale squares sit at the top of the coefficient range, at the lowest block shift: what the
    # coupling sum (and the rematrixing sum and difference) takes in from up to five channels (5.1 `rails` reaches 23 552)
    for i in (1, 5, 6):
        assert np.abs(mdct[i, :, :, :nfbw].astype(np.int64)).max() >= 23000 and (shift[i, :, :, :nfbw] == -9).all()
    assert nch == 2 or np.abs(mdct[1].astype(np.int64)).max() == 23552


@pytest.mark.parametrize("nch", [2, 6])
def test_block_switch_decisions(strict, nch):
    pcm = T.corner_batch(nch)
    nfbw = min(nch, 5)
    for i, kind in enumerate(T.CORNER_KINDS):
        sw = B.decisions(pcm[i], T.chmap_of(nch), nfbw)
        assert int(sw.sum()) == BLKSW[kind][nch == 6], (kind, int(sw.sum()))
        if kind in FULL_SCALE:
            assert sw[0, 0].all()                                   # the first block of every full-bandwidth channel, alone
        if kind == "onset":
            assert sw[1, 2].all()                                   # 1536 + 700 = block 2 of frame 1


@pytest.mark.parametrize("nch", [2, 6])
def test_drc_words(strict, nch):
    pcm = T.corner_batch(nch)
    nfbw = min(nch, 5)
    for i, kind in enumerate(T.CORNER_KINDS):
        codes, snt, _, _ = D.encode(pcm[i], T.chmap_of(nch), nfbw, 1, 24)
        got = (int(snt.sum()), int(codes.min()), int(codes.max()))
        assert got == DRC[kind][nch == 6], (kind, got)
        assert (got[0] == 6 * F) == (kind in FULL_SCALE)
        assert -128 <= got[1] and got[2] <= 127


def test_rematrixing_flags(strict, stages):
    """the window table is served by the built library without a device, so the 2/0 flags are pinned here"""
    pcm, mdct, shift = stages[2]
    exact = 0
    for i, kind in enumerate(T.CORNER_KINDS):
        v = R.block_v(pcm[i], (0, 1))
        assert np.array_equal(v - 9, shift[i][:, :, :2]), kind      # the model's block exponent is the reference's shift
        rows, sh, flags, rs = R.rematrix(mdct[i][:, :, :2], v)
        assert rs[:, 0].all() and set(np.unique(flags)) <= set(range(16))
        if kind in REMAT:
            assert flags.tolist() == REMAT[kind], (kind, flags.tolist())
            exact += 1
        else:
            assert flags.any(), kind
        if not flags.any():
            assert np.array_equal(rows, mdct[i][:, :, :2])
    assert exact == len(REMAT)
