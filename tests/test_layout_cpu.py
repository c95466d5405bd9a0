"""CPU: the encoder layout setter's boundary (ac3mi_set_encode_layout) and tests/layout_model.py's restatements."""
import os

from tests import _harness as H
from tests import layout_model as M


def test_setter_is_declared_and_exported():
    pkg = H.pkg()
    assert "ac3mi_set_encode_layout" in pkg.declared_symbols()
    assert hasattr(pkg.load_library(), "ac3mi_set_encode_layout")
    assert hasattr(pkg.Engine, "set_encode_layout")
    hdr = open(os.path.join(H.ROOT, "include", "ac3mi.h")).read()
    doc = hdr[:hdr.index("int ac3mi_set_encode_layout(")]
    doc = doc[doc.rindex("/*"):]
    for word in ("dialnorm2", "dynrng2e", "nfchans(acmod) + lfeon", "AC3MI_DOLBY", "mode 0"):
        assert word in doc, word


def test_reference_table_and_counts():
    assert [M.channels(*M.REF_LAYOUT[n]) for n in range(1, 7)] == [1, 2, 3, 4, 5, 6]
    assert sorted(M.channels(a, l) for a, l in M.layouts()) == sorted([2, 1, 2, 3, 3, 4, 4, 5, 3, 2, 3, 4, 4, 5, 5, 6])


def test_granted_layouts():
    assert M.granted_layout(2) == (2, 0)
    assert M.granted_layout(M.A52_DOLBY) == (2, 0)
    assert M.granted_layout(M.A52_CHANNEL1) == (1, 0)
    assert M.granted_layout(M.A52_CHANNEL2) == (1, 0)
    assert M.granted_layout(0) == (0, 0)
    assert M.granted_layout(7 | 16) == (7, 1)
    assert M.granted_layout(2 | 16) == (2, 1)


def test_follow_map_inverts_the_interleave():
    """Coded channel k of the new frames is WAVE slot follow_map[k]; the converter put plane wave_planes[w] in slot w, so
    the composition must give decoded coded channel k's plane (lfe + k, the LFE plane 0)."""
    for flags in [a | l for a in range(8) for l in (0, 16)] + [8, 9, 10, 8 | 16, 10 | 16]:
        acmod, lfeon = M.granted_layout(flags)
        planes = M.wave_planes(flags)
        fm = M.follow_map(flags)
        assert sorted(fm) == list(range(len(planes)))
        nf = M.NFCHANS[acmod]
        assert [planes[w] for w in fm] == [lfeon + k for k in range(nf)] + [0] * lfeon, flags
    # 5.1: WAVE order L R C LFE Ls Rs; coded L C R Ls Rs LFE
    assert M.follow_map(7 | 16) == [0, 2, 1, 4, 5, 3]
    # 2/1+LFE: WAVE L R LFE S
    assert M.follow_map(4 | 16) == [0, 1, 3, 2]
