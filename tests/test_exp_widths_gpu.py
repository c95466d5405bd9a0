"""GPU: the encoder's exponent coding (csrc/enc_exp.h) at every width a row can have.  What depends on the width is which
entry is a row's last - the lane it falls in and where in the lane - and with it the carries of the +-2 constraint across
the 16-lane rows of the DPP network: a channel's rows at every chbwcod 0..50 (n = 73 + 3 chbwcod) with the reference's
strategies and the cost-based ones, and the coupling channel's at every cplbegf, to the default end and to the shortest and
longest range the bandwidth tool gives it.  The models and checkers are those of tests/test_exp_strategy_gpu.py."""
import numpy as np
import pytest

from tests import _tools as T
from tests import bandwidth_model as W
from tests import exp_strategy_model as X

pytestmark = pytest.mark.gpu

PER = {1: 4, 2: 2, 3: 1}        # a lane's entries of a channel's row by strategy (D15, D25, D45)


def _check_mode0_rows(t0, nch, n):
    """A strategy-mode-0 call at n coded bins: the exponents sent are bandwidth_model.encode_exp on the call's own raw
    exponents and strategies (the LFE: 7 bins)."""
    S, F = t0["exponent"].shape[:2]
    for s in range(S):
        for f in range(F):
            for ch in range(nch):
                hi = 7 if nch == 6 and ch == 5 else n
                want = W.encode_exp(t0["exponent"][s, f, :, ch], t0["exp_strategy"][s, f, :, ch], hi)
                assert np.array_equal(t0["encoded_exp"][s, f, :, ch, :hi], want), (n, s, f, ch)


def test_channel_rows_at_every_width(engine):
    """Mono, an attack and a noise stream of one frame, at every chbwcod the encoder offers, 0..50 (ac3mi_set_encode_bandwidth
    refuses 51..60, legal in A/52: the packers' member lists are sized for 223 coefficients a channel - so n = 226..253 cannot
    be reached, and the refusal is asserted instead); 5.1 at chbwcod 50, the LFE's seven bins with it.  Both strategy modes
    against their models.  The sweep must have coded D15, D25, D45 and reuse, and rows whose last entry lies in the last lane
    of one 16-lane row and in the first lane of the next."""
    for c in range(51, 61):
        with pytest.raises(Exception):
            engine.set_encode_bandwidth(1, c)
    cases = [(1, c) for c in range(51)] + [(6, 50)]
    seen = set()                # (entries of the row, strategy) of every set sent by a full-bandwidth channel; (0, 0): reuse
    for nch, c in cases:
        pcm = np.concatenate([T.content("attack", nch, 1, 1, seed=31), T.content("noise", nch, 1, 1, seed=32)])
        n = W.nbc(c)
        _, t1 = T.encode(engine, pcm, xs=1, bw=(1, c), taps=True)
        _, t0 = T.encode(engine, pcm, xs=0, bw=(1, c), taps=True)
        T.check_rows(t1, nch, n)
        _check_mode0_rows(t0, nch, n)
        for t in (t0, t1):
            for st in np.unique(t["exp_strategy"][:, :, :, :min(nch, 5)]):
                seen.add((3 * X.groups(n, int(st)), int(st)) if st else (0, 0))
    assert {s for _, s in seen} == {0, 1, 2, 3}, sorted({s for _, s in seen})
    last = {s: {(ng - 1) // PER[s] for ng, s_ in seen if s_ == s} for s in (1, 2, 3)}      # the lane of the last entry
    print("lanes of a row's last entry by strategy:", {s: sorted(v) for s, v in last.items()})
    assert any({15, 16} <= v or {31, 32} <= v for v in last.values())


def _cpl_cases(begf):
    """(chbwcod or None) of the coupling ranges of one cplbegf: the default end (217), and with bandwidth mode 1 the shortest
    and the longest legal range (cplendf = min(12, chbwcod >> 2), begf <= cplendf + 2; the longest is the default's, reached
    through the kernels that take the end at run time)."""
    return (None, 4 * max(0, begf - 2), 50)


def test_coupling_row_at_every_start(engine):
    """2/0, three music streams and one with identical channels, one frame: every cplbegf with each of _cpl_cases' ends,
    both strategy modes (tests/_tools.check_coupled_frames).  Every range must have met a coupled frame (when written, and
    with the build before csrc/enc_exp.h, all four frames couple in each of the 39)."""
    pcm = np.concatenate([T.content("music", 2, 3, 1, seed=41), T.content("identical", 2, 1, 1, seed=45)])
    counts = {}
    for begf in range(13):
        counts[begf] = [T.check_coupled_frames(engine, pcm, 2, begf, c, mode0=True) for c in _cpl_cases(begf)]
    print("coupled frames of %d by cplbegf (default end, shortest, longest range):" % pcm.shape[0], counts)
    assert all(n > 0 for v in counts.values() for n in v), counts
