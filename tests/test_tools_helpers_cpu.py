"""CPU: the frame views of tests/_tools.py on what is available without a GPU, the oracle encoder's frames (uncoupled, full
bandwidth, default metadata), and on those frames with BSI bits rewritten.  tests/packer.py draws chincpl, phsflginu and
cplbndstrc at random and does not report what it wrote, so it cannot supply coupled frames that meet the views' structural
assertions; the coupled side is held by the GPU tests against tests/coupling_model.py."""
import numpy as np
import pytest

from tests import _harness as H
from tests import _tools as T

DEFAULTS = dict(bsid=8, bsmod=0, cmixlev=1, surmixlev=1, dsurmod=0, dialnorm=31, copyrightb=0, origbs=1)


@pytest.fixture(scope="module")
def frames():
    return {nch: H.orc_encode(H.gen_pcm(2, nch, seed=17 + nch, kind="music"), nch, T.RATE[nch],
                              chmap=(T.chmap_of(nch) + (0,) * 8)[:8]) for nch in (1, 2, 6)}


@pytest.mark.parametrize("nch", [1, 2, 6])
def test_block0_views_on_oracle_frames(frames, nch):
    for fr in frames[nch]:
        assert T.coupling_view(fr, nch) == (0, None, None, None, None)
        rm = []
        assert T.coupling_view(fr, nch, remat=rm)[0] == 0 and rm == []
        # (the reference sends rematstr with four zero flags in block 0 of a 2/0 frame)
        assert T.uncoupled_view(fr, nch) == (0 if nch == 2 else None, [50] * min(nch, 5))
    rs, fl = T.remat_view(frames[2])
    assert rs.shape == fl.shape == (2,) and rs.all() and not fl.any()
    with pytest.raises(AssertionError):
        T.uncoupled_view(frames[nch][0], 2 if nch != 2 else 6)         # acmod is the expected one


@pytest.mark.parametrize("nch", [1, 2, 6])
def test_bsi_view_on_oracle_frames(frames, nch):
    acmod = T.ACMOD[nch]
    present = {"cmixlev": (acmod & 1) and acmod != 1, "surmixlev": acmod & 4, "dsurmod": acmod == 2}
    widths = [(k, n) for k, n in T.METADATA_WIDTHS if present.get(k, k != "dialnorm2")]
    for fr in frames[nch]:
        fields, where = T.bsi_view(fr)
        assert fields["acmod"] == acmod and fields["lfeon"] == (nch == 6)
        assert {k: v for k, v in fields.items() if k in DEFAULTS} == {k: v for k, v in DEFAULTS.items() if present.get(k, True)}
        assert all(fields[k] == 0 for k in T.BSI_OPTIONS if k in fields) and "compre" in fields and "addbsie" in fields
        # the positions: exactly the metadata fields' widths, ascending, bsmod first (after syncinfo and bsid), and the
        # bits there are the fields' values
        assert len(where) == sum(n for _, n in widths) and where == sorted(set(where)) and where[0] == 45
        bits = np.unpackbits(fr)
        p = 0
        for k, n in widths:
            assert int("".join(str(b) for b in bits[where[p:p + n]]), 2) == fields[k], k
            p += n
        # rewritten metadata is read back, at the same positions; nothing else changes
        bits[where] ^= 1
        f2, w2 = T.bsi_view(np.packbits(bits))
        assert w2 == where and all(f2[k] == fields[k] ^ ((1 << n) - 1) for k, n in widths)
        assert {k: v for k, v in f2.items() if k not in dict(widths)} == {k: v for k, v in fields.items() if k not in dict(widths)}
        # an optional BSI field (compre, the bit after dialnorm) is refused
        bits = np.unpackbits(fr)
        i = [k for k, _ in widths].index("dialnorm")
        bits[where[sum(n for _, n in widths[:i])] + 5] = 1
        with pytest.raises(AssertionError):
            T.bsi_view(np.packbits(bits))
