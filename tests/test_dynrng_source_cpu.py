"""CPU: tests/dynrng_model.py - the rule of ac3mi_set_encode_dynrng_frames / ac3mi_set_encode_drc_source - on hand-written
cases and on packer streams, and the two entry points in the header and the library."""
import numpy as np
import pytest

from tests import _harness as H
from tests import ac3_syntax as A
from tests import dynrng_model as D
from tests import packer


def _raw(words):
    """{(block, programme): word} -> raw [6][2]"""
    raw = np.zeros((6, 2), np.int64)
    for (b, p), w in words.items():
        raw[b, p] = 0x100 | w
    return raw


def test_a_word_in_block_3_only():
    codes = D.in_force(_raw({(3, 0): 0x47}))
    assert codes[:, 0].tolist() == [0, 0, 0, 0x47, 0x47, 0x47] and not codes[:, 1].any()
    assert D.sends(codes)[:, 0].tolist() == [False, False, False, True, False, False]
    assert [D.gain(c) for c in codes[:, 0]] == [1.0] * 3 + [D.gain(0x47)] * 3 and D.gain(0x47) != 1.0


def test_a_word_repeated_unchanged_is_sent_once():
    codes = D.in_force(_raw({(1, 0): 0xe3, (2, 0): 0xe3, (4, 0): 0xe3}))
    assert codes[:, 0].tolist() == [0, 0xe3, 0xe3, 0xe3, 0xe3, 0xe3]
    assert D.sends(codes)[:, 0].tolist() == [False, True, False, False, False, False]


def test_word_0_in_block_0_sends_nothing():
    """word 0 is gain 1.0, the gain every frame starts at: the new frame need not say so; a later return to 0 is sent"""
    assert D.gain(0) == 1.0
    codes = D.in_force(_raw({(0, 0): 0}))
    assert not codes.any() and not D.sends(codes).any()
    codes = D.in_force(_raw({(0, 0): 0, (2, 0): 0x21, (4, 0): 0}))
    assert codes[:, 0].tolist() == [0, 0, 0x21, 0x21, 0, 0]
    assert D.sends(codes)[:, 0].tolist() == [False, False, True, False, True, False]


def test_dual_mono_programmes_are_independent():
    codes = D.in_force(_raw({(0, 0): 0x10, (2, 1): 0xf0, (5, 0): 0x11, (5, 1): 0xf0}))
    assert codes[:, 0].tolist() == [0x10] * 5 + [0x11] and codes[:, 1].tolist() == [0, 0, 0xf0, 0xf0, 0xf0, 0xf0]
    s = D.sends(codes)
    assert s[:, 0].tolist() == [True, False, False, False, False, True] and s[:, 1].tolist() == [False, False, True, False, False, False]
    # sends works on whole batches too
    batch = np.stack([codes, np.zeros_like(codes)])[None]
    assert np.array_equal(D.sends(batch)[0, 0], s) and not D.sends(batch)[0, 1].any()


LAYOUTS = [(0, 0, 20), (1, 0, 16), (2, 0, 20), (7, 1, 30)]


@pytest.mark.parametrize("acmod,lfeon,frmsizecod", LAYOUTS)
def test_hold_and_reset_on_packer_streams(acmod, lfeon, frmsizecod):
    """a word holds to the end of its frame and no further: every frame starts again at 0"""
    F = 6
    src = np.stack([packer.make_stream(4200 + 10 * acmod + s, F, acmod, lfeon, frmsizecod=frmsizecod,
                                       features=dict(dynrng=0.5, bsi_opts=0.5)) for s in range(2)])
    parsed = [[A.parse_frame(fr) for fr in st] for st in src]
    nprog = 2 if acmod == 0 else 1
    first = [P.blocks[0].fields["dynrnge"] for st in parsed for P in st]
    assert 0 < sum(first) < len(first), "the seeds give frames with and without a word in block 0"
    assert any(P.fields["compre"] for st in parsed for P in st), "the seeds give a compr word"
    codes, compr = D.effective(src)
    assert codes.shape == (2, F, 6, 2) and compr.shape == (2, F, 2)
    ended_nonzero_then_silent = 0
    for s in range(2):
        for f in range(F):
            P = parsed[s][f]
            for p, sfx in enumerate(("", "2")[:nprog]):
                e = 0
                for b in range(6):
                    if P.blocks[b].fields["dynrng%se" % sfx]:
                        e = P.blocks[b].fields["dynrng" + sfx]
                    assert codes[s, f, b, p] == e, (s, f, b, p)
                if not P.blocks[0].fields["dynrng%se" % sfx]:
                    assert codes[s, f, 0, p] == 0
                    ended_nonzero_then_silent += f > 0 and codes[s, f - 1, 5, p] != 0
                assert compr[s, f, p] == (0x100 | P.fields["compr" + sfx] if P.fields["compr%se" % sfx] else 0)
            if nprog == 1:
                assert not codes[s, f, :, 1].any() and compr[s, f, 1] == 0
    assert ended_nonzero_then_silent > 0, "no frame tests the reset"
    # a damaged frame carries nothing, its neighbours theirs
    status = np.zeros((2, F), np.uint32)
    status[0, 1], status[1, 2], status[1, 4] = 0x13f, 0x4, 0xc00
    c2, k2 = D.effective(src, status)
    assert not c2[0, 1].any() and not c2[1, 2].any() and not k2[0, 1].any() and not k2[1, 2].any()
    keep = np.ones((2, F), bool)
    keep[0, 1] = keep[1, 2] = False
    assert np.array_equal(c2[keep], codes[keep]) and np.array_equal(k2[keep], compr[keep])
    if acmod == 0:
        # one programme of a dual-mono source coded as something else
        for prog in (0, 1):
            c1, k1 = D.effective(src, prog=prog)
            assert np.array_equal(c1[..., 0], codes[..., prog]) and not c1[..., 1].any()
            assert np.array_equal(k1[..., 0], compr[..., prog]) and not k1[..., 1].any()
        assert not np.array_equal(codes[..., 0], codes[..., 1])


def test_entry_points_are_declared_and_exported():
    pkg = H.pkg()
    lib = pkg.load_library()
    names = pkg.declared_symbols()
    for n in ("ac3mi_set_encode_dynrng_frames", "ac3mi_set_encode_drc_source"):
        assert n in names and hasattr(lib, n), n
    assert lib.ac3mi_set_encode_dynrng_frames(None, None, None) == -1 and lib.ac3mi_set_encode_drc_source(None, 0) == -1
    flags = __import__(pkg.__name__ + ".flags", fromlist=["x"])
    assert (flags.DRC_SOURCE_CONTEXT, flags.DRC_SOURCE_FOLLOW, flags.COMPR_SENT) == (0, 1, 0x100)
