"""CPU gate of the decoder conformance matrix (tests/_decode_matrix.py): the thirteen cases build to the frame sizes the list
names, still carry the features they are there for, decode without error under every output request, and the liba52
restatement that the GPU tests compare with equals the real liba52 on them."""
import numpy as np
import pytest

from tests import _decode_matrix as M
from tests import _harness as H
from tests import ac3_syntax as A
from tests import packer

# per case, out of the 144 blocks of its 24 frames: half of the smallest count measured over the thirteen cases when the list
# was drawn up (coupling 78, short blocks 38, delta bit allocation 47, skip fields 36, dynrng words 40, rematrix flags 60)
FLOORS = dict(cplinu=39, blksw=19, deltbaie=23, skiple=18, dynrnge=20, rematflg=30)


def _frames(case):
    return np.concatenate([M.multi(case).reshape(-1, M.CASES[case]), M.single(case).reshape(-1, M.CASES[case])])


@pytest.mark.parametrize("case", M.CASE_LIST, ids=M.case_id)
def test_case_builds_and_carries_its_features(case):
    acmod, lfe, fscod, bsid, fsz = case
    assert M.multi(case).shape == (M.MULTI_S, M.MULTI_F, M.CASES[case]) and M.single(case).shape == (M.SINGLE_S, 1, M.CASES[case])
    assert packer.frame_bytes(fscod, fsz) == M.CASES[case]
    n = dict.fromkeys(FLOORS, 0)
    for fr in _frames(case):
        P = A.parse_frame(fr)                                  # read to the end by the independent reader
        assert (P.acmod, P.lfeon, P.fscod, P.bsid, P.frame_bytes) == (acmod, lfe, fscod, bsid, M.CASES[case])
        for B in P.blocks:
            n["cplinu"] += int(bool(B.cplinu))
            n["blksw"] += int(any(v for k, v in B.fields.items() if k.startswith("blksw")))
            n["rematflg"] += int(any(v for k, v in B.fields.items() if k.startswith("rematflg")))
            for k in ("deltbaie", "skiple", "dynrnge"):
                n[k] += int(B.fields[k])
    print("%s: of 144 blocks %r" % (M.case_id(case), n))
    for k, floor in FLOORS.items():
        if (k == "cplinu" and acmod < 2) or (k == "rematflg" and acmod != 2):
            continue                   # (the packer couples from acmod 2 up: mono has nothing to couple, dual mono's two are programmes)
        assert n[k] >= floor, (k, n[k], floor)


@pytest.mark.parametrize("case", M.CASE_LIST, ids=M.case_id)
def test_restatement_decodes_every_request(case):
    """no error under any request, with the LFE, and under the layout request with A52_ADJUST_LEVEL, other levels and dynrng
    off; the grant is the request, but for the 2/0 sources, where the frame's dsurmod decides between STEREO and DOLBY"""
    acmod = case[0]
    layout = M.requests(case)[0]
    grants = set()
    for frames in (M.multi(case), M.single(case)):
        for req in M.requests(case):
            st = M.liba52_stages((case, frames.shape[1]), frames, acmod, req)
            g = st["flags"] & 15
            if acmod == 2 and (req & 15) in (2, 10):
                grants |= set(g.ravel().tolist())
                assert set(g.ravel().tolist()) <= {2, 10}
            elif acmod == 1 and (req & 15) == 2:
                assert (g == 10).all(), (req, g)               # a52_downmix_init's table: mono to two channels is DOLBY
            else:
                assert (g == (req & 15)).all(), (req, g)
            assert ((st["flags"] & 16) == (req & 16)).all()
        for kw in (dict(flags=layout | M.ADJUST_LEVEL), dict(flags=layout, level=0.5), dict(flags=layout, level=2.0),
                   dict(flags=layout, dynrng_off=True), dict(flags=layout, bias=384.0)):
            status, pcm, whole = H.orc_decode_status(frames, **kw)
            assert not status.any() and (whole == frames.shape[1]).all() and np.isfinite(pcm).all()
    if acmod == 2:
        assert grants == {2, 10}, "the matrix holds both STEREO and DOLBY grants"


def test_restatement_arguments_decide_something():
    """level scales the PCM, dynrng off changes it, a seeded state changes the first block and the dither: the arguments that
    H.orc_decode_status gained are in effect (its defaults are what every earlier caller got)"""
    case = (0, 0, 1, 9, 25)
    frames = M.multi(case)
    _, base, _ = H.orc_decode_status(frames, 0)
    _, half, _ = H.orc_decode_status(frames, 0, level=0.5)
    assert np.allclose(half, 0.5 * base, rtol=1e-6, atol=1e-9) and np.abs(base).max() > 0
    _, flat, _ = H.orc_decode_status(frames, 0, dynrng_off=True)
    assert not np.array_equal(flat, base)
    delay, lfsr = M.mid_run_state(frames.shape[0], 2, 3)
    _, seeded, _ = H.orc_decode_status(frames, 0, state=(delay, lfsr))
    assert not np.array_equal(seeded[:, 0, 0], base[:, 0, 0])
    zero = (np.zeros_like(delay), np.ones_like(lfsr))
    assert np.array_equal(H.orc_decode_status(frames, 0, state=zero)[1].view(np.uint32), base.view(np.uint32))


@pytest.mark.parametrize("case", M.CASE_LIST, ids=M.case_id)
def test_restatement_equals_liba52(case):
    """stream 0 of the multi-frame batch, the layout request and the 2/0 (or mono) downmix, bit for bit: against liba52
    itself where oracle/_ref exists, else against its results in tests/golden/liba52_records.json"""
    fr = np.ascontiguousarray(M.multi(case)[0])
    for flags in (M.requests(case)[0], M.downmix_request(case)):
        want = H.ref_decode_record(fr, flags, 1.0, 0.0)
        got = H.decode_record(*H.orc_decode(fr, flags, 1.0, 0.0))
        assert want[1] == 0 and got[1] == 0 and got[2] == want[2]
        assert got == want, (case, flags)


@pytest.mark.parametrize("case", M.DAMAGED_CASES, ids=M.case_id)
def test_damaged_frames_build(case):
    """fuzz_corrupt.make_damaged builds at the three sizes the GPU test runs, and its damage makes blocks fail"""
    from tests import fuzz_corrupt
    acmod, lfe, fscod, bsid, fsz = case
    frames, _, want_fail, want_foreign, _ = fuzz_corrupt.make_damaged(M.DAMAGED_SEED, acmod, lfe, fscod=fscod, bsid=bsid, frmsizecod=fsz)
    assert frames.shape == (96, M.CASES[case]) and (want_fail < 6).sum() > 0 and (want_fail[:6] == 6).all()


@pytest.mark.parametrize("case", M.tail_cases(), ids=M.case_id)
def test_overrun_frames_read_behind_their_end(case):
    """_decode_matrix.overrun: the restatement decodes them without error, to other samples in the last block than the frames
    they were made from, and in several of them the last block's mantissas begin inside the frame and end behind the two bytes
    that follow it - so those two bytes are mantissa bits to a decoder that takes them for the frame's"""
    frames, start = M.overrun(case)
    acmod, fb = case[0], M.CASES[case]
    assert fb % 4 == 2 and frames.shape[0] >= 3
    status, pcm, whole = H.orc_decode_status(frames, M.requests(case)[0])
    assert not status.any() and (whole == 1).all() and np.isfinite(pcm).all()
    crossing = 0
    for s, fr in enumerate(frames):
        buf = np.zeros(fb + 64, np.uint8)
        buf[:fb] = fr[0]
        end = packer._end_of_block(H.orc(), buf, 5, acmod)
        crossing += int(start[s] <= fb * 8 and end >= fb * 8 + 16)
    print("%s: %d frames with a lengthened skip field in the last block, in %d its mantissas cross the two bytes behind the frame" % (
        M.case_id(case), len(frames), crossing))
    assert crossing >= 3


@pytest.mark.parametrize("case", M.CASE_LIST, ids=M.case_id)
def test_forgotten_bias_names_the_streams_it_should(case):
    """_decode_matrix.forgotten_bias against the restatement at bias 384: a stream has blocks that went out without the bias -
    samples within +-100 of zero where everything else lies around 384 - exactly where the helper says liba52 forgets it, and
    the matrix holds such streams (two)"""
    frames = M.multi(case)
    for req in M.requests(case):
        _, pcm, _ = H.orc_decode_status(frames, req, 384.0)
        # a whole plane of a block without the bias: its mean is the signal's, near 0, not near 384
        bare = (np.abs(pcm.mean(axis=-1)) < 100.0).any(axis=(1, 2, 3))
        assert np.array_equal(bare, M.forgotten_bias(case, frames, req, 384.0)), (req, bare)
        assert not M.forgotten_bias(case, frames, req, 0.0).any()
    if case in ((4, 1, 2, 8, 26), (6, 1, 1, 9, 35)):
        assert M.forgotten_bias(case, frames, 2 | 16, 384.0).sum() == 1
