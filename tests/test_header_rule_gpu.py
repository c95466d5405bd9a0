"""GPU: one refusal rule for every kernel that reads a frame's head.  Two batches of one-frame streams (tests/packer.py) - 2/0 at
48 kHz, frmsizecod 20, in slots of 768 bytes, and the small 5.1 + LFE layout the fixed-shape kernels take - in which stream 0 is
as packed and every other stream has header bytes edited and nothing else (EDITS below).  Which streams are refused comes from
tests/stream_model.syncinfo_size, the slot size and the call's acmod / lfeon, nothing from the engine: every decoder front end
(ac3mi_set_decode_mode 1, 3, 4, 5, 6 and the rule, with and without the fixed-shape kernels) sets status bit 0x100 on exactly
those streams, the CRC kernel of a decode call sums exactly the others, and ac3mi_crc_check_batch, ac3mi_bsi_read_batch and
ac3mi_frame_scan_batch, which do not test acmod / lfeon, refuse exactly what the header test or the slot size refuses.

No tolerance is this file's own: the front ends among themselves are byte-identical (_decode_matrix.same), the accepted streams
are held to the liba52 restatement by _decode_matrix.held_to_liba52."""
import os

import numpy as np
import pytest

from tests import _decode_matrix as M
from tests import _harness as H
from tests import crc_model, packer
from tests.stream_model import syncinfo_size

pytestmark = pytest.mark.gpu

# (acmod, lfeon, fscod, bsid, frmsizecod) -> the slot, and the (fscod, frmsizecod) of four of the edits
CASES = {
    (2, 0, 0, 8, 20): dict(slot=768, twin=(0, 21), smaller=(0, 18), short_other_rate=(1, 18), long_other_rate=(2, 20)),
    M.FIXED_SHAPE_CASE: dict(slot=976, twin=(1, 22), smaller=(1, 21), short_other_rate=(0, 23), long_other_rate=(2, 23)),
}
CASE_LIST = list(CASES)
SEED0 = 9700
ALL = pytest.mark.parametrize("case", CASE_LIST, ids=M.case_id)


def _lfeon_at(acmod):
    """bit of the frame at which lfeon lies: behind acmod and the two-bit cmixlev, surmixlev, dsurmod that acmod sends"""
    return 48 + 3 + 2 * (int(bool(acmod & 1) and acmod != 1) + int(bool(acmod & 4)) + int(acmod == 2))


def _acmod_lfeon(fr):
    acmod = int(fr[6]) >> 5
    at = _lfeon_at(acmod)
    return acmod, (int(fr[at >> 3]) >> (7 - (at & 7))) & 1


def _sizecod(fr, fscod, code):
    fr[4] = fscod << 6 | code


def _flip_lfeon(fr):
    at = _lfeon_at(int(fr[6]) >> 5)
    fr[at >> 3] ^= 0x80 >> (at & 7)


def _edits(case):
    """name -> (the edit of a frame's header bytes, whether the rule, the slot and the call then accept the frame)"""
    c = CASES[case]
    fscod = case[2]
    return [
        ("untouched", lambda fr: None, True),
        ("sync word 0x0b76", lambda fr: fr.__setitem__(1, 0x76), False),
        ("byte 5 0x60", lambda fr: fr.__setitem__(5, 0x60), False),
        ("bsid 11", lambda fr: fr.__setitem__(5, 0x58 | (int(fr[5]) & 7)), True),
        ("frmsizecod 37", lambda fr: _sizecod(fr, fscod, 37), False),
        ("frmsizecod 38", lambda fr: _sizecod(fr, fscod, 38), False),
        ("frmsizecod 63", lambda fr: _sizecod(fr, fscod, 63), False),
        ("fscod 3", lambda fr: _sizecod(fr, 3, case[4]), False),
        ("the twin frmsizecod", lambda fr: _sizecod(fr, *c["twin"]), True),
        ("a smaller frmsizecod", lambda fr: _sizecod(fr, *c["smaller"]), True),
        ("another fscod, too long for the slot", lambda fr: _sizecod(fr, *c["long_other_rate"]), False),
        ("another fscod, short", lambda fr: _sizecod(fr, *c["short_other_rate"]), True),
        ("acmod changed", lambda fr: fr.__setitem__(6, (int(fr[6]) & 0x1f) | ((case[0] ^ 1) << 5)), False),
        ("lfeon flipped", _flip_lfeon, False),
    ]


_BUILT = {}


def batch(case):
    """-> (frames [S][1][slot] read-only, names, rule [S]: the header test passes and the frame fits its slot, accepted [S]: and
    its acmod / lfeon are the call's).  Needs no GPU."""
    if case not in _BUILT:
        acmod, lfe, fscod, bsid, code = case
        fb = CASES[case]["slot"]
        assert packer.frame_bytes(fscod, code) == fb
        edits = _edits(case)
        frames = np.stack([packer.make_stream(SEED0 + 31 * s + acmod, 1, acmod, lfe, fscod=fscod, bsid=bsid, frmsizecod=code)
                           for s in range(len(edits))])
        rule, accepted = [], []
        for s, (name, edit, want) in enumerate(edits):
            before = frames[s, 0].copy()
            edit(frames[s, 0])
            assert (frames[s, 0, 8:] == before[8:]).all() and ((frames[s, 0] != before).any() or s == 0), name
            own = syncinfo_size(frames[s, 0, :8].tolist())
            rule.append(0 < own <= fb)
            accepted.append(rule[-1] and _acmod_lfeon(frames[s, 0]) == (acmod, lfe))
            assert accepted[-1] == want, (name, own)
        sizes = [syncinfo_size(fr[0, :8].tolist()) for fr in frames]
        assert sizes[8] in (fb, fb - 2) and sizes[9] < fb - 2 and sizes[11] < fb - 2 and fb < sizes[10] and fb < sizes[4]
        frames.setflags(write=False)
        _BUILT[case] = (frames, [e[0] for e in edits], np.array(rule), np.array(accepted))
    return _BUILT[case]


def reference(case, flags, bias=0.0):
    """the liba52 restatement on the batch: it refuses exactly the expected streams and decodes block 0 of every other one (a
    condition on the batch: a frame that reuses state at block 0 may differ between batch shapes)"""
    frames, names, _, accepted = batch(case)
    ref = M.liba52(("header rule", case), frames, flags, bias)
    assert np.array_equal(ref[0][:, 0] == 0x13f, ~accepted), (ref[0][:, 0], accepted)
    assert not (ref[0][accepted, 0] & 1).any(), [names[s] for s in np.nonzero(ref[0][:, 0] & 1)[0]]
    return ref


def _restore(engine):
    engine.set_decode_mode(int(os.environ.get("AC3MI_DECODE_MODE", "0")))
    engine.set_fixed_shape(1)
    engine.set_decode_crc(0)


def _refusals(got, accepted, names, what):
    status = got["status"][:, 0].astype(np.uint32)
    refused = (status & 0x100) != 0
    assert np.array_equal(refused, ~accepted), (what, [names[s] for s in np.nonzero(refused == accepted)[0]])
    assert not (status[accepted] & 0x200).any(), (what, [names[s] for s in np.nonzero(status & 0x200)[0]])


@ALL
def test_every_front_end_refuses_the_same_streams(engine, case):
    """with stage taps, modes 1, 3, 4, 5: status, coefficient planes, block-switch flags, PCM and state byte-identical; without,
    modes 4, 5, 6 and the rule against mode 1, float and s16, the 5.1 batch with the generic kernels as well; mode 1 held to the
    restatement; bit 0x100 on exactly the expected streams and bit 0x200 on no accepted one, in every one of them"""
    frames, names, _, accepted = batch(case)
    flags = M.requests(case)[0]
    try:
        base = None
        for mode in (1, 3, 4, 5):
            engine.set_decode_mode(mode)
            got = M.decode(engine, frames, case, flags, taps=True)
            _refusals(got, accepted, names, "%s mode %d with taps" % (M.case_id(case), mode))
            if base is None:
                base = got
                print("%s: float RMS %.3g of level, peak %.3g of peak" % ((M.case_id(case),) + M.held_to_liba52(
                    got, reference(case, flags), reference(case, flags)[2])))
            M.same(got, base, "mode %d against mode 1, with taps" % mode)
        for s16 in (False, True):
            engine.set_decode_mode(1)
            base = M.decode(engine, frames, case, flags, s16=s16)
            ref = reference(case, flags, 384.0 if s16 else 0.0)
            M.held_to_liba52(base, ref, ref[2], s16)
            for mode in (3, 4, 5, 6, 0):
                engine.set_decode_mode(mode)
                for fixed in ((1, 0) if case == M.FIXED_SHAPE_CASE else (1,)):
                    engine.set_fixed_shape(fixed)
                    what = "%s mode %d%s%s" % (M.case_id(case), mode, " s16" if s16 else "", "" if fixed else ", generic kernels")
                    got = M.decode(engine, frames, case, flags, s16=s16)
                    _refusals(got, accepted, names, what)
                    M.same(got, base, what + " against mode 1")
                engine.set_fixed_shape(1)
    finally:
        _restore(engine)


@ALL
def test_crc_kernel_sums_what_the_front_ends_accept(engine, case):
    """The CRC kernel of a decode call runs with the call's acmod / lfeon, and its verdict byte shows in status bits 10 / 11.
    The packer's CRC words are random, so every frame that is summed fails (the model says in which regions).

    ac3mi_set_decode_crc 2 is the run that shows what was summed: a frame that fails gets bit 6 of its verdict, the front ends
    then refuse it, and bit 6 lets bits 10 / 11 of a refused frame through.  So every stream carries bit 0x100, the accepted ones
    carry the model's bits, and a stream the rule, the slot or acmod / lfeon refuses carries neither bit only if the CRC kernel
    left it out (verdict 0x80) - summed by mistake, 'acmod changed' or 'lfeon flipped' would fail and show its bits here.
    (Checked against a scratch build whose crc_kernel does not test lfeon: both cases fail here, in the first mode, on 'lfeon
    flipped', status 0xd3f where 0x13f is due; every other test of this file passes on it.)
    Under ac3mi_set_decode_crc 1 the front ends mask bits 10 / 11 of any frame they refuse themselves, so that run holds the
    accepted streams' bits and the refusals only.
    ac3mi_crc_check_batch takes no layout: verdict 0x80 exactly where the header test or the slot size refuses, the model's
    elsewhere."""
    import torch
    frames, names, rule, accepted = batch(case)
    fb = frames.shape[2]
    model = crc_model.verdicts(frames[:, 0], fb)
    assert np.array_equal(model == crc_model.NOT_SUMMED, ~rule) and (model & 3)[rule].all()
    want = np.where(accepted, (model & 3).astype(np.uint32) << 10, 0)
    try:
        for mode in (1, 3, 4, 5, 6, 0):
            engine.set_decode_mode(mode)
            engine.set_decode_crc(2)
            got = M.decode(engine, frames, case, M.requests(case)[0])
            status = got["status"][:, 0].astype(np.uint32)
            assert np.array_equal(status & 0xc00, want), (mode, [names[s] for s in np.nonzero((status & 0xc00) != want)[0]])
            assert ((status & 0x13f) == 0x13f).all(), (mode, [names[s] for s in np.nonzero((status & 0x13f) != 0x13f)[0]])
            engine.set_decode_crc(1)
            got = M.decode(engine, frames, case, M.requests(case)[0])
            bits = got["status"][:, 0].astype(np.uint32) & 0xc00
            assert np.array_equal(bits, want), (mode, [names[s] for s in np.nonzero(bits != want)[0]])
            _refusals(got, accepted, names, "%s mode %d under ac3mi_set_decode_crc 1" % (M.case_id(case), mode))
    finally:
        _restore(engine)
    verdict = engine.crc_check_batch(torch.from_numpy(M.pad(frames)).cuda(), fb)
    engine.sync()
    verdict = verdict.cpu().numpy()[:, 0]
    assert np.array_equal(verdict, model), [names[s] for s in np.nonzero(verdict != model)[0]]


@ALL
def test_bsi_reader_and_frame_scan_follow_the_rule(engine, case):
    """ac3mi_bsi_read_batch: AC3MI_BSI_NOT_READ exactly where the header test or the slot size refuses; it reads the two streams
    of another acmod / lfeon, and echoes every read head's fields.  ac3mi_frame_scan_batch, mode 0, every slot a stream of
    frame_bytes bytes: a frame at offset 0, of the header's size, exactly on the same streams."""
    import torch
    pkg = H.pkg()
    frames, names, rule, accepted = batch(case)
    S, _, fb = frames.shape
    assert (rule & ~accepted).sum() == 2
    info = engine.bsi_read_batch(torch.from_numpy(M.pad(frames)).cuda(), fb)
    engine.sync()
    info = info.cpu().numpy().view(pkg.capi.bsi_info_dtype())[:, 0, 0]
    not_read = (info["verdict"] & pkg.flags.BSI_NOT_READ) != 0
    assert np.array_equal(not_read, ~rule), [names[s] for s in np.nonzero(not_read == rule)[0]]
    for s in np.nonzero(rule)[0]:
        fr = frames[s, 0]
        assert (info["fscod"][s], info["frmsizecod"][s], info["bsid"][s]) == (fr[4] >> 6, fr[4] & 63, fr[5] >> 3), names[s]
        assert (info["acmod"][s], info["lfeon"][s]) == _acmod_lfeon(fr), names[s]

    stride = (fb + 15) & ~15
    buf = np.zeros((S, stride), np.uint8)
    buf[:, :fb] = frames[:, 0]
    refs, sinfo = engine.frame_scan_batch(torch.from_numpy(buf).cuda(), torch.full((S,), fb, dtype=torch.int32, device="cuda"), 0, 8)
    engine.sync()
    refs = refs.cpu().numpy().view(pkg.capi.frame_ref_dtype())[..., 0]
    n_frames = sinfo.cpu().numpy().view(pkg.capi.scan_info_dtype())[..., 0]["n_frames"]
    for s in range(S):
        own = syncinfo_size(frames[s, 0, :8].tolist())
        at0 = [(int(r["offset"]), int(r["bytes"])) for r in refs[s, :min(1, int(n_frames[s]))] if r["offset"] == 0]
        assert at0 == ([(0, own)] if rule[s] else []), (names[s], at0, own)
