"""GPU: every decoder front end on batches whose frames differ in size (tests/_mixed_sizes.py; tests/test_mixed_sizes_cpu.py
pins the inputs): 44.1 kHz streams, whose frames alternate between the sizes of an odd and an even frmsizecod, in both phases
in one batch, and a batch of six streams of three sample rates and five bit rates, as ac3mi_frame_gather_batch lays them out.
Every frame lies in a slot of the batch's largest size; include/ac3mi.h: "every frame starts on its frame_stride slot and
carries its own size" - what a frame decodes to is a function of its own bytes, and what lies behind them in its slot reads as
zero, as it does to the liba52 restatement, to frame_gather_kernel and to crc_kernel.

The modes are those of tests/test_decode_matrix_gpu.py (ac3mi_set_decode_mode 1, 3, 4, 5, 6 and the rule, 0), and so are the
bars: no tolerance is this file's own.  Integer stages and coefficient planes are exact, float and s16 PCM are held to the
restatement by _decode_matrix.held_to_liba52's rule, the front ends among themselves are byte-identical.  Every decode of (a)
to (c) runs with the slots' tails filled with 0x00, with 0xff and with random bytes, and must give the same bytes (d.i)."""
import os

import numpy as np
import pytest

from tests import _decode_matrix as M
from tests import _harness as H
from tests import _mixed_sizes as X

pytestmark = pytest.mark.gpu

ALL = pytest.mark.parametrize("case", X.CASE_LIST, ids=X.case_id)
TRANSCODE_CASES = [c for c in X.CASE_LIST if c[2] in "BC"]
GATHER_CASES = [c for c in X.CASE_LIST if c[2] in "AC"]


def _restore(engine):
    engine.set_decode_mode(int(os.environ.get("AC3MI_DECODE_MODE", "0")))
    engine.set_fixed_shape(1)
    engine.set_decode_crc(0)
    engine.set_encode_metadata_source(0)
    engine.set_encode_drc_source(0)
    engine.set_encode_metadata_frames(None)
    engine.set_encode_dynrng_frames(None, None)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _whole(frames):
    return np.full(frames.shape[0], frames.shape[1])


def _any_fill(engine, case, which, flags, what, **kw):
    """(d.i) one decode per tail fill, byte-identical in pcm, status, delay and lfsr (and the taps); the 0x00 one"""
    res = [M.decode(engine, X.laid(case, which, fill), case, flags, **kw) for fill in X.FILLS]
    for fill, r in zip(X.FILLS[1:], res[1:]):
        M.same(r, res[0], "%s: slot tails of %r against zeros" % (what, fill))
    return res[0]


def _stages_hold(got, want, case, what):
    """status, final dither state, block-switch flags (where the restatement has them) and coefficient planes exactly the
    restatement's, float PCM within the bar"""
    acmod, lfe = case[:2]
    nf = H.NFCHANS[acmod]
    assert (got["status"] & 0x1ff).max() == 0, (what, got["status"])
    assert np.array_equal((got["status"] >> 16) & 0xff, want["flags"]), (what, got["status"] >> 16, want["flags"])
    assert np.array_equal(got["lfsr"].astype(np.int64) & 0xffff, want["lfsr"]), (what, got["lfsr"], want["lfsr"])
    assert np.array_equal(got["blksw"][..., :nf], want["blksw"][..., :nf]), what
    # (the restatement's planes and the engine's both hold the LFE first: the request carries it whenever the source does)
    differ = _bits(got["coef"]) != _bits(want["coef"][:, :, :, :nf + lfe])
    assert not differ.any(), "%s: coefficient planes differ in %d values, first (stream, frame, block, plane, bin) %r" % (
        what, differ.sum(), np.argwhere(differ)[0].tolist())
    err = got["pcm"].astype(np.float64) - want["pcm"]
    scale_rms, scale_max = max(1.0, H.rms(want["pcm"])), max(1.0, float(np.abs(want["pcm"]).max()))
    print("%s: RMS error %.3g of level %.3g, peak error %.3g of peak %.3g" % (what, H.rms(err), scale_rms, np.abs(err).max(), scale_max))
    assert H.rms(err) <= 1e-6 * scale_rms and np.abs(err).max() <= 1e-5 * scale_max, what


def _figures(s16, fig):
    return "s16 largest step %d, RMS %.3g of level" % fig if s16 else "float RMS %.3g of level, peak %.3g of peak" % fig


# ---------------------------------------------------------------------------------------------------------------------
# a. stages

@ALL
def test_stages(engine, case):
    """the multi batch with stage taps under the layout request: mode 1 exactly the restatement's stages, modes 3, 4, 5
    byte-identical to mode 1; every one of them whatever the slots' tails hold"""
    flags = M.requests(case)[0]
    want = M.liba52_stages((case, "multi"), X.laid(case, "multi"), case[0], flags)
    res = {}
    try:
        for mode in (1, 3, 4, 5):
            engine.set_decode_mode(mode)
            res[mode] = _any_fill(engine, case, "multi", flags, "%s stages mode %d" % (X.case_id(case), mode), taps=True)
    finally:
        _restore(engine)
    _stages_hold(res[1], want, case, "%s stages" % X.case_id(case))
    for mode in (3, 4, 5):
        M.same(res[mode], res[1], "mode %d against mode 1" % mode)


# ---------------------------------------------------------------------------------------------------------------------
# b. requests and s16

@ALL
def test_requests(engine, case):
    """the multi batch without taps, the layout request and the downmix request, float and s16: mode 4 held to the restatement,
    modes 6 and 0 byte-identical to it; the layout request once more from overlap tails and dither states of streams in
    mid-run.  (None of these requests is one of _decode_matrix.forgotten_bias: the plain mix is liba52's.)"""
    frames = X.laid(case, "multi")
    S = frames.shape[0]
    layout = M.requests(case)[0]
    n_out = H.NFCHANS[case[0]] + case[1]
    variants = [(req, s16, None) for req in (layout, M.downmix_request(case)) for s16 in (False, True)]
    variants += [(layout, s16, M.mid_run_state(S, n_out, 700 + case[0])) for s16 in (False, True)]
    try:
        for req, s16, state in variants:
            what = "%s request %d%s%s" % (X.case_id(case), req, " s16" if s16 else "", " from mid-run state" if state else "")
            assert not M.forgotten_bias(case, frames, req, 384.0 if s16 else 0.0).any()
            engine.set_decode_mode(4)
            base = _any_fill(engine, case, "multi", req, what + " mode 4", s16=s16, state=state)
            assert base["pcm"].any()
            ref = M.liba52((case, "multi"), frames, req, 384.0 if s16 else 0.0, state=state)
            print("%s: %s" % (what, _figures(s16, M.held_to_liba52(base, ref, _whole(frames), s16))))
            for mode in (6, 0):
                engine.set_decode_mode(mode)
                M.same(_any_fill(engine, case, "multi", req, what + " mode %d" % mode, s16=s16, state=state), base,
                       "%s: mode %d against mode 4" % (what, mode))
    finally:
        _restore(engine)


# ---------------------------------------------------------------------------------------------------------------------
# c. one-frame streams

@ALL
def test_one_frame_streams(engine, case):
    """the nine one-frame streams under the layout request - the identity, so mode 6 takes mantx_kernel -, float and s16: mode 1
    held to the restatement, modes 3, 4, 6 and 0 byte-identical to mode 1.  The 5.1 case takes the fixed-shape kernels; it runs
    with ac3mi_set_fixed_shape 0 as well: the generic instantiations give the same bytes."""
    frames = X.laid(case, "single")
    flags = M.requests(case)[0]
    try:
        for s16 in (False, True):
            what = "%s one-frame streams%s" % (X.case_id(case), " s16" if s16 else "")
            engine.set_decode_mode(1)
            base = _any_fill(engine, case, "single", flags, what + " mode 1", s16=s16)
            ref = M.liba52((case, "single"), frames, flags, 384.0 if s16 else 0.0)
            print("%s: %s" % (what, _figures(s16, M.held_to_liba52(base, ref, _whole(frames), s16))))
            for mode in (3, 4, 6, 0):
                engine.set_decode_mode(mode)
                for fixed in ((1, 0) if case == X.FIXED_SHAPE_CASE else (1,)):
                    engine.set_fixed_shape(fixed)
                    how = "%s mode %d%s" % (what, mode, "" if fixed else ", generic kernels")
                    M.same(_any_fill(engine, case, "single", flags, how, s16=s16), base, how + " against mode 1")
                engine.set_fixed_shape(1)
    finally:
        _restore(engine)


# ---------------------------------------------------------------------------------------------------------------------
# d. the slot's tail is not the frame  (d.i is _any_fill, in every mode of a to c)

@ALL
def test_bytes_behind_a_short_frame_are_not_the_frame(engine, case):
    """(d.ii) tests/test_decode_matrix_gpu.py::test_bytes_behind_a_frame_are_not_the_frame where a frame's own size is below the
    batch's frame_bytes: short frames whose last block's mantissas begin in the frame's own last byte and run on behind it
    (_mixed_sizes.overrun_short), each behind a full-size frame, the slots' tails 0x00, 0xff and random.  The restatement reads
    zeros behind a frame's own end, so the engine must not take the slot's bytes for mantissa bits: planes exact and PCM within
    the bar in modes 1, 3, 4, 5; without taps modes 6 and 0 byte-identical to mode 4, float and s16; no result depends on the
    fill.

    Before the staging loops of decode_kernel.h, decode_wg.hip, mant_kernel and mantx_kernel trimmed a staged frame to its own
    size, this failed in all four cases at its first comparison with a fill other than zeros - mode 1, tails 0xff: case A's
    coefficient planes differed in 62 values, the first in block 5 of the short frame of stream 0 (B: 85, C: 1043, D: 38) -
    while tails of 0x00 passed in every mode, and so did every other test of this file."""
    flags = M.requests(case)[0]
    zeros = X.laid(case, "overrun", 0)
    want = M.liba52_stages((case, "overrun"), zeros, case[0], flags)
    try:
        for fill in X.FILLS:
            frames = X.laid(case, "overrun", fill)
            for mode in (1, 3, 4, 5):
                engine.set_decode_mode(mode)
                got = M.decode(engine, frames, case, flags, taps=True)
                _stages_hold(got, want, case, "%s overrunning short frames, tails %r, mode %d" % (X.case_id(case), fill, mode))
        for s16 in (False, True):
            ref = M.liba52((case, "overrun"), zeros, flags, 384.0 if s16 else 0.0)
            base = None
            for fill in X.FILLS:
                frames = X.laid(case, "overrun", fill)
                what = "%s overrunning short frames%s, tails %r" % (X.case_id(case), " s16" if s16 else "", fill)
                engine.set_decode_mode(4)
                got = M.decode(engine, frames, case, flags, s16=s16)
                print("%s: %s" % (what, _figures(s16, M.held_to_liba52(got, ref, _whole(frames), s16))))
                if base is None:
                    base = got
                M.same(got, base, what + " against zeros")
                for mode in (6, 0):
                    engine.set_decode_mode(mode)
                    M.same(M.decode(engine, frames, case, flags, s16=s16), base, "%s: mode %d against mode 4" % (what, mode))
    finally:
        _restore(engine)


# ---------------------------------------------------------------------------------------------------------------------
# e. too long for the slot

@ALL
def test_a_frame_too_long_for_the_slot(engine, case):
    """a short frame whose header says a size above frame_bytes (only its frmsizecod edited), the last of its stream: status
    0x100 | 0x3f and what any refused frame gets - the bytes of the same call with that frame's sync word zeroed instead:
    silence behind the fading overlap, zero tails, the dither state that of the stream's frames before it (the
    restatement's) -; every other stream's bytes those of the call without the edit; the stream's earlier frames held to
    the restatement."""
    src, s = X.too_long(case)
    edited = X.lay_edited(src, X.slot(case), 0xff)
    clean = X.laid(case, "multi", 0xff)
    nosync = edited.copy()
    nosync[s, -1, :2] = 0
    flags = M.requests(case)[0]
    ref = M.liba52((case, "too long"), edited, flags)
    before = M.liba52_stages((case, "before"), np.ascontiguousarray(clean[:, :-1]), case[0], flags)
    assert ref[0][s, -1] == 0x13f and np.count_nonzero(ref[0]) == 1
    others = np.arange(edited.shape[0]) != s
    try:
        for mode in (1, 3, 4, 5, 0):
            engine.set_decode_mode(mode)
            what = "%s mode %d" % (X.case_id(case), mode)
            got = M.decode(engine, edited, case, flags)
            assert (got["status"][s, -1] & 0x1ff) == 0x100 | 0x3f, (what, hex(got["status"][s, -1]))
            M.held_to_liba52(got, ref, ref[2], False)
            assert not got["pcm"][s, -1, 1:].any() and not got["delay"][s].any(), what
            assert (int(got["lfsr"][s]) & 0xffff) == before["lfsr"][s], (what, got["lfsr"][s], before["lfsr"][s])
            M.same(got, M.decode(engine, nosync, case, flags), what + ": against the frame without a sync word")
            plain = M.decode(engine, clean, case, flags)
            M.same({k: v[others] for k, v in got.items()}, {k: v[others] for k, v in plain.items()}, what + ": the other streams")
            assert np.array_equal(got["pcm"][s, :-1], plain["pcm"][s, :-1]) and plain["pcm"][s, -1, 1:].any()
    finally:
        _restore(engine)


# ---------------------------------------------------------------------------------------------------------------------
# f. gathered streams

@pytest.mark.parametrize("case", GATHER_CASES, ids=X.case_id)
def test_scan_gather_decode(engine, case):
    """the streams of the multi batch as byte streams, a few bytes without a sync word between some of their frames:
    ac3mi_frame_scan_batch (mode 0), ac3mi_frame_gather_batch at the case's slot size and ac3mi_decode_s16_batch give the bytes
    of the same call on the frames laid out by the host with zeros behind them (tests/test_frame_scan_gpu.py's
    test_scan_gather_decode, whose frames are all of one size)"""
    import torch
    pkg = H.pkg()
    src = X.streams(case, "multi")
    S, F, fb = len(src), X.MULTI_F, X.slot(case)
    data = [X.byte_stream(st, 50 + s) for s, st in enumerate(src)]
    assert any(len(d) > sum(len(fr) for fr in st) for d, st in zip(data, src))
    stride = (max(len(d) for d in data) + 15) & ~15
    buf = np.zeros((S, stride), np.uint8)
    for s, d in enumerate(data):
        buf[s, :len(d)] = d
    lens = np.array([len(d) for d in data], np.int32)
    d_buf = torch.from_numpy(buf).cuda()
    refs, info = engine.frame_scan_batch(d_buf, torch.from_numpy(lens).cuda(), 0, 8)
    gathered = engine.frame_gather_batch(d_buf, refs, info, F, fb)
    engine.sync()
    n_frames = info.cpu().numpy().view(pkg.capi.scan_info_dtype())[..., 0]["n_frames"]
    assert [int(n) for n in n_frames] == [F] * S
    host = np.zeros((S, F, gathered.shape[2]), np.uint8)
    host[:, :, :fb] = X.laid(case, "multi", 0)
    assert np.array_equal(gathered.cpu().numpy(), host)
    flags = M.requests(case)[0]
    desc = pkg.DecodeDesc(flags=flags, level=1.0, bias=384.0, dynrng=1, acmod=case[0], lfeon=case[1], frame_bytes=fb)
    n_out, _ = engine.decode_planes(desc)
    res = []
    for fr_t in (gathered, torch.from_numpy(host).cuda()):
        delay = torch.zeros((S, n_out, 128), dtype=torch.float32, device="cuda")
        lfsr = torch.ones((S,), dtype=torch.int16, device="cuda")
        pcm, status = engine.decode_s16_batch(desc, fr_t, delay, lfsr)
        engine.sync()
        res.append((pcm.cpu().numpy(), status.cpu().numpy(), delay.cpu().numpy(), lfsr.cpu().numpy()))
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    assert not (res[0][1] & 0x13f).any()
    # and these are the bytes of the decode calls of (b)
    base = M.decode(engine, X.laid(case, "multi", 0xff), case, flags, s16=True)
    assert np.array_equal(res[0][0], base["pcm"]) and np.array_equal(res[0][3], base["lfsr"])


# ---------------------------------------------------------------------------------------------------------------------
# g. transcode

def _transcode_calls(engine, frames, fb, case, crc=0):
    """-> (ac3mi_transcode_batch following its source's BSI and dynamic-range words, ac3mi_decode_s16_batch + ac3mi_encode_batch
    given those words by tests/bsi_model.py and tests/dynrng_model.py): two dicts of frames, status and the four state arrays"""
    import torch
    from tests import bsi_model, dynrng_model
    pkg = H.pkg()
    S, F, _ = frames.shape
    acmod, lfe = case[:2]
    dec = pkg.DecodeDesc(flags=acmod | 16 * lfe, level=1.0, bias=384.0, dynrng=0, acmod=acmod, lfeon=lfe, frame_bytes=fb)
    n_out, _ = engine.decode_planes(dec)
    enc = pkg.EncodeDesc(48000, 448000, n_out)
    d_frames = torch.from_numpy(M.pad(frames)).cuda()

    def state():
        return (torch.zeros((S, n_out, 128), dtype=torch.float32, device="cuda"), torch.ones((S,), dtype=torch.int16, device="cuda"),
                torch.zeros((S, n_out, 256), dtype=torch.int16, device="cuda"), torch.full((S,), 40, dtype=torch.int32, device="cuda"))

    def host(out, status, st):
        return dict(frames=out.cpu().numpy(), status=status.cpu().numpy(), delay=st[0].cpu().numpy(), lfsr=st[1].cpu().numpy(),
                    last=st[2].cpu().numpy(), csnr=st[3].cpu().numpy())

    engine.set_decode_crc(crc)
    engine.set_encode_metadata_source(1)
    engine.set_encode_drc_source(1)
    st = state()
    out, status = engine.transcode_batch(dec, enc, d_frames, st[0], st[1], H.CHMAP6, st[2], st[3])
    engine.sync()
    got = host(out, status, st)
    engine.set_encode_metadata_source(0)
    engine.set_encode_drc_source(0)
    ctx_word = bsi_model.pack_word()
    words = np.array([[bsi_model.followed_word(bsi_model.parse_head(fr), acmod, ctx_word) for fr in stream] for stream in frames], np.int64)
    codes, compr = dynrng_model.effective(frames)
    assert dynrng_model.sends(codes).sum() > S * F and (compr & 0x100).any() and len(np.unique(words)) > 1, "the sources carry words"
    st = state()
    pcm, status = engine.decode_s16_batch(dec, d_frames, st[0], st[1])
    engine.set_encode_metadata_frames(torch.from_numpy(words.astype(np.uint32).view(np.int32)).cuda())
    engine.set_encode_dynrng_frames(torch.from_numpy(np.ascontiguousarray(codes, np.uint8)).cuda(),
                                    torch.from_numpy(np.ascontiguousarray(compr).astype(np.uint16).view(np.int16)).cuda())
    out = engine.encode_batch(enc, pcm.view(S, F, 1536, n_out), H.CHMAP6, st[2], st[3])
    engine.sync()
    engine.set_encode_metadata_frames(None)
    engine.set_encode_dynrng_frames(None, None)
    return got, host(out, status, st)


@pytest.mark.parametrize("which", ["multi", "single"])
@pytest.mark.parametrize("case", TRANSCODE_CASES, ids=X.case_id)
def test_transcode_equals_the_calls(engine, case, which):
    """the 5.1 cases, frames with both CRC words right (crc_model.seal) and random bytes behind them:
    ac3mi_transcode_batch under ac3mi_set_encode_metadata_source 1 and ac3mi_set_encode_drc_source 1 - its BSI and
    dynamic-range readers meet frames shorter than frame_bytes - equals ac3mi_decode_s16_batch + ac3mi_encode_batch given each
    frame's words, byte for byte and state for state (tests/test_transcode_gpu.py's test_transcode_equals_the_three_calls).
    Under ac3mi_set_decode_crc 1 bits 10 and 11 stay clear, the bytes the same; with the last own byte of one short frame
    flipped, that frame alone gets AC3MI_STATUS_CRC2."""
    CRC1, CRC2 = H.pkg().flags.STATUS_CRC1, H.pkg().flags.STATUS_CRC2
    fb = X.slot(case)
    frames = X.lay(X.sealed(case, which), fb, "random")
    try:
        got, want = _transcode_calls(engine, frames, fb, case)
        assert (got["status"] & 0x1ff).max() == 0
        for k in want:
            assert np.array_equal(got[k], want[k]), "%s %s: `%s` of the transcode is not that of the two calls" % (X.case_id(case), which, k)
        checked, _ = _transcode_calls(engine, frames, fb, case, crc=1)
        for k in got:
            assert np.array_equal(checked[k], got[k]), "%s %s: `%s` under ac3mi_set_decode_crc 1" % (X.case_id(case), which, k)
        s, f = next((s, f) for s, st in enumerate(X.sealed(case, which)) for f, fr in enumerate(st) if len(fr) < fb)
        hit = frames.copy()
        hit[s, f, len(X.sealed(case, which)[s][f]) - 1] ^= 0x01
        flagged, _ = _transcode_calls(engine, hit, fb, case, crc=1)
        want_bits = np.zeros_like(got["status"])
        want_bits[s, f] = CRC2
        assert np.array_equal(flagged["status"] & (CRC1 | CRC2), want_bits), (flagged["status"] & (CRC1 | CRC2), s, f)
        assert (flagged["status"] & 0x1ff).max() == 0
    finally:
        _restore(engine)
