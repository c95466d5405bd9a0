"""GPU: every decoder front end against the liba52 restatement on the conformance matrix of tests/_decode_matrix.py - thirteen
packer layouts at 32, 44.1 and 48 kHz, bsid 8, 9 and 10, frames of 192 to 3 840 bytes (two of them 2 mod 4), every acmod, with
coupling, rematrixing, phase flags, block switching, delta bit allocation, skip fields, dynrng / dynrng2 words and optional
BSI fields (tests/test_decode_matrix_cpu.py pins the list and holds the restatement to liba52 itself on it).

ac3mi_set_decode_mode: 1 = one wavefront per stream (decode_kernel<0>), 3 = one workgroup per stream (decode_wg.hip), 4 / 5 = the
split front end parsed per stream / per frame + mant_kernel + xform_kernel, 6 = the split front end + mantx_kernel, 0 = the
rule of capi.hip.  Auto hands every call of up to 512 streams of at most four frames to the workgroup kernel, so the modes are
forced here, and auto is run on both sides of its thresholds.

No tolerance is this file's own: the integer stages and the coefficient planes are exact, float PCM is held to 1e-6 of
max(1, level) RMS and 1e-5 of max(1, peak), s16 PCM to the rule of _decode_matrix.held_to_liba52 - all against the
restatement; the front ends among themselves are byte-identical.  Every test prints the worst figures it saw."""
import os

import numpy as np
import pytest

from tests import _decode_matrix as M
from tests import _harness as H
from tests import variant_matrix as V

pytestmark = pytest.mark.gpu

ALL = pytest.mark.parametrize("case", M.CASE_LIST, ids=M.case_id)


def _restore(engine):
    engine.set_decode_mode(int(os.environ.get("AC3MI_DECODE_MODE", "0")))
    engine.set_fixed_shape(1)


FRONT = {1: [V.dec(0)], 4: [V.dec(4), V.MANT], 5: [V.dec(5), V.LFSR, V.MANT]}


def _forced(engine, mode, frames, case, flags, **kw):
    """M.decode under ac3mi_set_decode_mode `mode` - and the call launched that mode's front end (ac3mi_debug_launch_log): 1, 4
    and 5 their kernels exactly, 3 the one-workgroup-per-stream kernel alone, 6 the per-stream parse kernel and then
    mantx_kernel where the call is one it fuses (one-frame streams, no downmix, no taps), else mant_kernel"""
    engine.set_decode_mode(mode)
    with V.tap(engine) as log:
        got = M.decode(engine, frames, case, flags, **kw)
    if mode in FRONT:
        assert log == FRONT[mode], (mode, log)
    elif mode == 3:
        assert len(log) == 1 and V.families(log) == {"decode_wg_kernel"}, log
    elif mode == 6:
        fuses = frames.shape[1] == 1 and flags == M.requests(case)[0] and not kw.get("taps")
        assert len(log) == 2 and log[0].startswith("decode_kernel<4,") and log[1].startswith("mantx_kernel" if fuses else "mant_kernel"), log
    return got


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _whole(frames):
    return np.full(frames.shape[0], frames.shape[1])


# ---------------------------------------------------------------------------------------------------------------------
# a. stages

@ALL
def test_stages(engine, case):
    """the multi-frame batch with stage taps under the layout request, modes 1, 3, 4, 5: status, granted flags per frame, final
    dither state, block-switch flags and coefficient planes exactly the restatement's, float PCM within the bar; modes 3, 4, 5
    byte-identical to mode 1"""
    acmod, lfe = case[:2]
    nf = H.NFCHANS[acmod]
    frames = M.multi(case)
    flags = M.requests(case)[0]
    want = M.liba52_stages((case, "multi"), frames, acmod, flags)
    res = {}
    try:
        for mode in (1, 3, 4, 5):
            res[mode] = _forced(engine, mode, frames, case, flags, taps=True)
    finally:
        _restore(engine)
    got = res[1]
    assert (got["status"] & 0x1ff).max() == 0, got["status"]
    assert np.array_equal((got["status"] >> 16) & 0xff, want["flags"]), (got["status"] >> 16, want["flags"])
    assert np.array_equal(got["lfsr"].astype(np.int64) & 0xffff, want["lfsr"])
    assert np.array_equal(got["blksw"][..., :nf], want["blksw"][..., :nf])
    # (the restatement's planes and the engine's both hold the LFE first: the request carries it whenever the source does)
    assert np.array_equal(_bits(got["coef"]), _bits(want["coef"][:, :, :, :nf + lfe])), "coefficient planes differ"
    err = got["pcm"].astype(np.float64) - want["pcm"]
    scale_rms, scale_max = max(1.0, H.rms(want["pcm"])), max(1.0, float(np.abs(want["pcm"]).max()))
    print("%s stages: RMS error %.3g of level %.3g, peak error %.3g of peak %.3g" % (
        M.case_id(case), H.rms(err), scale_rms, np.abs(err).max(), scale_max))
    assert H.rms(err) <= 1e-6 * scale_rms and np.abs(err).max() <= 1e-5 * scale_max
    for mode in (3, 4, 5):
        M.same(res[mode], got, "mode %d against mode 1" % mode)


@pytest.mark.parametrize("case", M.tail_cases(), ids=M.case_id)
def test_bytes_behind_a_frame_are_not_the_frame(engine, case):
    """the two cases whose frames end in mid-dword, on frames whose last block's mantissas run on behind the frame
    (_decode_matrix.overrun; no undamaged frame reads that far): the restatement reads zeros there, so the engine must not take
    the 0xff that _decode_matrix.pad leaves between a frame's end and its slot's - the masked last dword of the four staging
    loops (decode_kernel.h: modes 1, 4, 5; decode_wg.hip: 3; decode.hip: mant_kernel; decode_mx.hip: mantx_kernel).  Planes
    exact and PCM within the bar in modes 1, 3, 4, 5; without taps, modes 6 and auto byte-identical to mode 4."""
    acmod, lfe = case[:2]
    nf = H.NFCHANS[acmod]
    frames, _ = M.overrun(case)
    flags = M.requests(case)[0]
    want = M.liba52_stages((case, "overrun"), frames, acmod, flags)
    try:
        for mode in (1, 3, 4, 5):
            got = _forced(engine, mode, frames, case, flags, taps=True)
            assert (got["status"] & 0x1ff).max() == 0, (mode, got["status"])
            assert np.array_equal(got["lfsr"].astype(np.int64) & 0xffff, want["lfsr"]), mode
            assert np.array_equal(_bits(got["coef"]), _bits(want["coef"][:, :, :, :nf + lfe])), "mode %d: coefficient planes differ" % mode
            err = got["pcm"].astype(np.float64) - want["pcm"]
            scale_rms, scale_max = max(1.0, H.rms(want["pcm"])), max(1.0, float(np.abs(want["pcm"]).max()))
            assert H.rms(err) <= 1e-6 * scale_rms and np.abs(err).max() <= 1e-5 * scale_max, (mode, H.rms(err), np.abs(err).max())
        for s16 in (False, True):
            engine.set_decode_mode(4)
            base = M.decode(engine, frames, case, flags, s16=s16)
            fig = M.held_to_liba52(base, M.liba52((case, "overrun"), frames, flags, 384.0 if s16 else 0.0), _whole(frames), s16)
            print("%s overrunning frames, %s" % (M.case_id(case),
                  "s16 largest step %d, RMS %.3g of level" % fig if s16 else "float RMS %.3g of level, peak %.3g of peak" % fig))
            for mode in (6, 0):
                engine.set_decode_mode(mode)
                M.same(M.decode(engine, frames, case, flags, s16=s16), base, "mode %d against mode 4" % mode)
    finally:
        _restore(engine)


# ---------------------------------------------------------------------------------------------------------------------
# b. requests

def _variants(case):
    """(request, s16, level, dynrng): every request in float and s16; the layout request with A52_ADJUST_LEVEL, at levels 0.5
    and 2 (float: the s16 call has no level) and with dynrng off - where the gain enters the parse kernel's descriptors"""
    reqs = M.requests(case)
    out = [(r, s16, 1.0, 1) for r in reqs for s16 in (False, True)]
    out += [(reqs[0] | M.ADJUST_LEVEL, s16, 1.0, 1) for s16 in (False, True)]
    out += [(reqs[0], False, 0.5, 1), (reqs[0], False, 2.0, 1)]
    out += [(reqs[0], s16, 1.0, 0) for s16 in (False, True)]
    return out


@ALL
def test_requests(engine, case):
    """the multi-frame batch without taps: the layout and every downmix liba52 grants from it, float at bias 0 and s16 at bias
    384.  Every variant runs; those that miss are reported together at the end.

    Under ac3mi_set_mix_state, which include/ac3mi.h names as what liba52's exact behaviour around frames with surround level
    0 takes (the drop-in and the stream layer always set it): mode 1 held to the restatement on every stream, modes 3, 4, 5
    and auto byte-identical to it - overlap tails, dither state and the mix state's two arrays included.

    Without it, the batched API's default, the plain linear mix: mode 1 held to the restatement as well, modes 3, 4, 5 and
    auto byte-identical to it - but for the PCM of the streams of _decode_matrix.forgotten_bias, where the header says the
    plain mix differs: at bias 384, in the path-A blocks of a frame with surmixlev "no surround", liba52 sends L and R of
    2/1, 2/2 -> STEREO and 3/1, 3/2 -> 3F out without the bias, and its converter turns them into rail values.
    Stream 4 of (4, 1, 2, 8, 26) and stream 3 of (6, 1, 1, 9, 35) are such streams: measured on MI355X, the plain mix differs
    from liba52 there in 9 and 16 of the 18 blocks by up to 65 535 steps (the rule allows 128 and 129), and the mix-state run
    holds.  Their status words are still held to the restatement's, and their state to the other modes'."""
    frames = M.multi(case)
    worst, missed = {}, []

    def hold(what, got, ref, first_bad, s16):
        try:
            worst[what] = (s16, M.held_to_liba52(got, ref, first_bad, s16))
        except AssertionError as e:
            missed.append("%s against the restatement (stream, largest error, allowed, RMS error, RMS level): %s" % (what, e.args[0]))

    try:
        for req, s16, level, dynrng in _variants(case):
            what = "request %d%s level %g dynrng %d" % (req, " s16" if s16 else "", level, dynrng)
            ref = M.liba52((case, "multi"), frames, req, 384.0 if s16 else 0.0, level, not dynrng)
            differs = M.forgotten_bias(case, frames, req, 384.0 if s16 else 0.0)
            for mix in (True, False):
                how = what + (", mix state" if mix else ", plain mix")
                base = _forced(engine, 1, frames, case, req, s16=s16, level=level, dynrng=dynrng, mix=mix)
                assert base["pcm"].any()
                hold(how, base, ref, _whole(frames) if mix else np.where(differs, 0, _whole(frames)), s16)
                for mode in (3, 4, 5, 0):
                    try:
                        M.same(_forced(engine, mode, frames, case, req, s16=s16, level=level, dynrng=dynrng, mix=mix), base,
                               "%s: mode %d against mode 1" % (how, mode))
                    except AssertionError as e:
                        missed.append(str(e))
            if differs.any():
                print("%s %s: the plain mix is not held to liba52's PCM on streams %s" % (M.case_id(case), what, np.flatnonzero(differs).tolist()))
    finally:
        _restore(engine)
    for what, (s16, fig) in worst.items():
        print("%s %s: %s" % (M.case_id(case), what,
              "s16 largest step %d, RMS %.3g of level" % fig if s16 else "float RMS %.3g of level, peak %.3g of peak" % fig))
    assert not missed, "\n".join(missed)


# ---------------------------------------------------------------------------------------------------------------------
# c. the fused mantissa + transform kernel

_FUSED = {}


def _single_state(case, S=M.SINGLE_S):
    n_out = H.NFCHANS[case[0]] + case[1]
    delay, lfsr = M.mid_run_state(M.SINGLE_S, n_out, 600 + case[0])
    idx = np.arange(S) % M.SINGLE_S
    return np.ascontiguousarray(delay[idx]), np.ascontiguousarray(lfsr[idx])


def _fused_reference(engine, case, s16):
    """mode 4 on the nine one-frame streams from the mid-run state, held to the restatement fed the same state; once"""
    if (case, s16) not in _FUSED:
        frames, flags, state = M.single(case), M.requests(case)[0], _single_state(case)
        base = _forced(engine, 4, frames, case, flags, s16=s16, state=state)
        ref = M.liba52((case, "single"), frames, flags, 384.0 if s16 else 0.0, state=state)
        fig = M.held_to_liba52(base, ref, _whole(frames), s16)
        print("%s one-frame streams from mid-run state, %s" % (M.case_id(case),
              "s16 largest step %d, RMS %.3g of level" % fig if s16 else "float RMS %.3g of level, peak %.3g of peak" % fig))
        _FUSED[(case, s16)] = base
    return _FUSED[(case, s16)]


@ALL
def test_fused_kernel(engine, case):
    """nine one-frame streams under the layout request - the identity, so mode 6 takes mantx_kernel - from overlap tails and
    dither states of streams in mid-run, float and s16: mode 4 held to the restatement, which starts from the same state (its
    overlap planes and generator seeded through H.orc_decode_status); mode 6 and auto byte-identical to mode 4.  The small 5.1
    case once more with ac3mi_set_fixed_shape 0: the FX instantiations against the generic ones on 976-byte 44.1 kHz frames."""
    frames, flags, state = M.single(case), M.requests(case)[0], _single_state(case)
    try:
        for s16 in (False, True):
            base = _fused_reference(engine, case, s16)
            for mode in (6, 0):
                M.same(_forced(engine, mode, frames, case, flags, s16=s16, state=state), base, "mode %d against mode 4" % mode)
                if case == M.FIXED_SHAPE_CASE:
                    engine.set_fixed_shape(0)
                    M.same(_forced(engine, mode, frames, case, flags, s16=s16, state=state), base, "mode %d, generic kernels, against mode 4" % mode)
                    engine.set_fixed_shape(1)
            # the state decided something: from new streams' state, other samples
            engine.set_decode_mode(4)
            assert not np.array_equal(M.decode(engine, frames, case, flags, s16=s16)["pcm"][:, 0, 0], base["pcm"][:, 0, 0])
    finally:
        _restore(engine)


# ---------------------------------------------------------------------------------------------------------------------
# d. calls

@ALL
def test_two_calls_equal_one(engine, case):
    """modes 4 and 5: frame 0 in one call, frames 1 and 2 in the next, the overlap tails and dither states carried from one to
    the other - the bytes of one call over the three; the layout in float and s16 and the first downmix in float"""
    frames = M.multi(case)
    head, tail = np.ascontiguousarray(frames[:, :1]), np.ascontiguousarray(frames[:, 1:])
    try:
        for mode in (4, 5):
            for req, s16 in ((M.requests(case)[0], False), (M.requests(case)[0], True), (M.downmix_request(case), False)):
                one = _forced(engine, mode, frames, case, req, s16=s16)
                a = _forced(engine, mode, head, case, req, s16=s16)
                b = _forced(engine, mode, tail, case, req, s16=s16, state=(a["delay"], a["lfsr"]))
                two = dict(pcm=np.concatenate([a["pcm"], b["pcm"]], axis=1), status=np.concatenate([a["status"], b["status"]], axis=1),
                           delay=b["delay"], lfsr=b["lfsr"])
                M.same(two, one, "mode %d request %d%s: two calls against one" % (mode, req, " s16" if s16 else ""))
                assert (one["status"] & 0x1ff).max() == 0
    finally:
        _restore(engine)


# ---------------------------------------------------------------------------------------------------------------------
# e. auto's thresholds

@pytest.mark.parametrize("case", M.THRESHOLD_CASES, ids=M.case_id)
def test_auto_thresholds(engine, case):
    """the bytes a caller gets do not depend on which side of a threshold of the front-end rule a batch lands: the nine
    one-frame streams tiled to 512 streams (the workgroup kernel) and to 513 (the split front end; to s16 with mantx_kernel),
    replica r the bytes of stream r % 9 and those the forced-mode result of test_fused_kernel; and the multi-frame batch
    lengthened to five frames a stream with its own frames (past four, the frame-parallel split front end) against mode 1"""
    frames, flags = M.single(case), M.requests(case)[0]
    try:
        for s16 in (False, True):
            base = _fused_reference(engine, case, s16)
            engine.set_decode_mode(0)
            for S in (512, 513):
                idx = np.arange(S) % M.SINGLE_S
                got = M.decode(engine, np.ascontiguousarray(frames[idx]), case, flags, s16=s16, state=_single_state(case, S))
                for k, v in got.items():
                    assert np.array_equal(v, v[idx]), "%d streams%s: `%s` of a replica is not its original's" % (S, " s16" if s16 else "", k)
                M.same({k: v[:M.SINGLE_S] for k, v in got.items()}, base, "auto on %d streams against mode 4 on nine" % S)
        multi = M.multi(case)
        longer = np.ascontiguousarray(np.concatenate([multi, multi[:, :2]], axis=1))
        for s16 in (False, True):
            engine.set_decode_mode(1)
            base = M.decode(engine, longer, case, flags, s16=s16)
            assert (base["status"] & 0x1ff).max() == 0
            engine.set_decode_mode(0)
            M.same(M.decode(engine, longer, case, flags, s16=s16), base, "auto on five frames a stream against mode 1")
    finally:
        _restore(engine)


# ---------------------------------------------------------------------------------------------------------------------
# f. damaged frames off the 48 kHz path

@pytest.mark.parametrize("case", M.DAMAGED_CASES, ids=M.case_id)
def test_damaged_frames(engine, case):
    """tests/fuzz_corrupt.py's round at 44.1 and 32 kHz sizes, modes 3, 4 and 5 (it takes taps, so mode 6 would not run its
    kernel): the restatement's first failing block, its planes before it and its dither state, frame by frame"""
    from tests import fuzz_corrupt
    acmod, lfe, fscod, bsid, fsz = case
    try:
        for mode, fill in ((3, 0x00), (4, 0xff), (5, 0xa5)):
            engine.set_decode_mode(mode)
            bad, failed, foreign = fuzz_corrupt.damaged_round(engine, M.DAMAGED_SEED, acmod, lfe, fill, fscod=fscod, bsid=bsid, frmsizecod=fsz)
            print("%s mode %d: %d frames failed a block, %d refused, %d mismatches" % (M.case_id(case), mode, failed, foreign, bad))
            assert bad == 0 and failed > 0
    finally:
        _restore(engine)
