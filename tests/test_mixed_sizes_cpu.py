"""CPU gate of the mixed-size decoder batches (tests/_mixed_sizes.py): the four cases build to the sizes their table names, both
sizes of a 44.1 kHz pair occur in every alternating stream and in both phases across streams, the liba52 restatement decodes
them whatever lies in the slots' tails, and the frames that tests/test_mixed_sizes_gpu.py needs for "the slot's tail is not the
frame" - short frames whose last block's mantissas run on behind the frame's own end - are there."""
import numpy as np
import pytest

from tests import _decode_matrix as M
from tests import _harness as H
from tests import _mixed_sizes as X
from tests import packer

ALL = pytest.mark.parametrize("case", X.CASE_LIST, ids=X.case_id)

SIZES = {"A": (834, 836), "B": (974, 976), "C": (1024, 1280, 1536, 1670, 1672, 1792), "D": (208, 210)}


@ALL
def test_sizes(case):
    """the sizes of the issue's table; both batches hold every one of them with the largest first; every stream that alternates
    holds both of its sizes, and at every frame position both phases occur across the streams"""
    acmod, lfe, name = case
    assert X.TABLE[name][3] == SIZES[name] and X.slot(case) == SIZES[name][-1]
    multi, single = X.streams(case, "multi"), X.streams(case, "single")
    assert len(multi) == len(X.TABLE[name][2]) and all(len(st) == X.MULTI_F for st in multi)
    assert len(single) == X.SINGLE_S and all(len(st) == 1 for st in single) and X.SINGLE_S % 8
    for batch in (multi, single):
        assert tuple(sorted({len(fr) for st in batch for fr in st})) == SIZES[name]
        assert len(batch[0][0]) == X.slot(case)
        for st in batch:
            for fr in st:
                assert X.own_size(fr) == len(fr) and (fr[6] >> 5) == acmod
    for (fscod, codes), st in zip(X.TABLE[name][2], multi):
        assert [len(fr) for fr in st] == [packer.frame_bytes(fscod, codes[f % len(codes)]) for f in range(X.MULTI_F)]
        if len(codes) == 2:
            assert len({len(fr) for fr in st}) == 2
    if name != "C":
        for f in range(X.MULTI_F):
            assert {len(st[f]) for st in multi} == set(SIZES[name]), "both phases at frame %d" % f
    assert X.laid(case, "multi").shape == (len(multi), X.MULTI_F, X.slot(case))
    assert X.laid(case, "single").shape == (X.SINGLE_S, 1, X.slot(case))


@ALL
def test_restatement_decodes_them_whatever_the_tail_holds(case):
    """status 0 under the layout request and the downmix request, and the same bits for slot tails of 0x00, 0xff and random
    bytes: the reference's contract - a frame is its own bytes, by its header's size"""
    for which in ("multi", "single"):
        for req in (M.requests(case)[0], M.downmix_request(case)):
            base = None
            for fill in X.FILLS:
                frames = X.laid(case, which, fill)
                status, pcm, whole = H.orc_decode_status(frames, req)
                assert not status.any() and (whole == frames.shape[1]).all() and np.isfinite(pcm).all() and pcm.any()
                if base is None:
                    base = pcm
                assert np.array_equal(pcm.view(np.uint32), base.view(np.uint32)), (which, req, fill)
    # the fills are not the same bytes
    a, b, c = (X.laid(case, "multi", fill) for fill in X.FILLS)
    assert not np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(b, c)


@ALL
def test_overrun_short_frames_read_behind_their_own_end(case):
    """_mixed_sizes.overrun_short: every frame is shorter than the slot and lies behind a full-size one; the restatement decodes
    the batch without error and to the same bits for every fill; and in at least three frames the last block's mantissas begin
    inside the frame and end 16 bits or more behind its own end - in bytes that are the slot's, not the frame's.  (A condition
    on the inputs, not a measurement: should a change of the packer break it, other seeds for the extra streams restore it.)"""
    src, start = X.overrun_short(case)
    acmod, fb = case[0], X.slot(case)
    assert all(len(st) == 2 and len(st[0]) == fb and len(st[1]) < fb for st in src)
    base = None
    for fill in X.FILLS:
        frames = X.laid(case, "overrun", fill)
        status, pcm, whole = H.orc_decode_status(frames, M.requests(case)[0])
        assert not status.any() and (whole == 2).all() and np.isfinite(pcm).all()
        if base is None:
            base = pcm
        assert np.array_equal(pcm.view(np.uint32), base.view(np.uint32)), fill
    crossing = 0
    for s, st in enumerate(src):
        own = len(st[1])
        buf = np.zeros(fb + 64, np.uint8)
        buf[:own] = st[1]
        end = packer._end_of_block(H.orc(), buf, 5, acmod)
        crossing += int(start[s] <= own * 8 and end >= own * 8 + 16)
    print("%s: %d short frames with a lengthened skip field in the last block, in %d its mantissas end at least 16 bits behind the frame's own end" % (
        X.case_id(case), len(src), crossing))
    assert crossing >= 3


@ALL
def test_a_frame_too_long_for_the_slot_is_refused(case):
    """only frmsizecod of a short frame edited, to a size above the slot: the restatement's harness refuses that frame (0x13f),
    the last of its stream, and decodes everything else"""
    src, s = X.too_long(case)
    clean = X.streams(case, "multi")
    assert np.flatnonzero(src[s][-1] != clean[s][-1]).tolist() == [4] and (src[s][-1][4] ^ clean[s][-1][4]) < 64
    frames = X.lay_edited(src, X.slot(case))
    status, pcm, whole = H.orc_decode_status(frames, M.requests(case)[0])
    want = np.zeros_like(status)
    want[s, -1] = 0x13f
    assert np.array_equal(status, want)
    assert np.array_equal(whole, np.where(np.arange(len(src)) == s, X.MULTI_F - 1, X.MULTI_F))
    _, ref, _ = H.orc_decode_status(X.laid(case, "multi"), M.requests(case)[0])
    assert np.array_equal(pcm[:, :-1].view(np.uint32), ref[:, :-1].view(np.uint32))
    assert not pcm[s, -1].any()
