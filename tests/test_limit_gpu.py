"""GPU: limit_kernel and limit_read_kernel (ac3mi_limit_batch, ac3mi_limit_read_batch) against tests/limit_model.py - the
limiter's rule in numpy int64 on tests/truepeak_model.py's interpolator - byte for byte: the output PCM and the state; their
independence of how a stream is cut into calls, of the buffers' alignment and of in-place use; bursts at the lane, delay,
frame and call seams; then end to end on decoded PCM with the meter behind it."""
import ctypes

import numpy as np
import pytest

from tests import _harness as H
from tests import _tools as T
from tests import limit_model as L
from tests import truepeak_model as M

pytestmark = pytest.mark.gpu

ERR_ARG = -1
C1, C2 = M.ceiling(-1.0), M.ceiling(-2.0)
R0 = 3496                               # ac3mi_limit_release_step(48000, 100.0)
NB = 1560


def _dev(pcm, offset=0):
    """int16 [S][n][C] -> a device tensor [S][F][1536][C] whose base lies `offset` int16 behind a 16-byte boundary"""
    import torch
    S, n, C = pcm.shape
    flat = torch.zeros(pcm.size + 8, dtype=torch.int16, device="cuda")
    assert flat.data_ptr() % 16 == 0
    t = flat[offset:offset + pcm.size]
    t.copy_(torch.from_numpy(np.ascontiguousarray(pcm).reshape(-1)))
    return t.view(S, n // 1536, 1536, C)


def _limit(engine, roles, C, R, pcm, cuts=None, offset=0, in_place=False, state=None):
    """the engine's limiter over pcm [S][n][C] in calls of `cuts` frames (default: one call), each call's buffers `offset` int16
    behind a 16-byte boundary -> (out int16 [S][n][C], the state tensor, its records, the result records)"""
    f, outs = 0, []
    for n in cuts or (pcm.shape[1] // 1536,):
        x = _dev(pcm[:, 1536 * f:1536 * (f + n)], offset)
        out = x if in_place else _dev(np.full((pcm.shape[0], 1536 * n, pcm.shape[2]), 0x5a5a, np.int16), offset)
        out, state = engine.limit_batch(roles, C, R, x, state, out)
        outs.append(out)
        f += n
    assert 1536 * f == pcm.shape[1]
    res = engine.limit_read_batch(state)
    engine.sync()
    out = np.concatenate([o.cpu().numpy().reshape(pcm.shape[0], -1, pcm.shape[2]) for o in outs], axis=1)
    return out, state, state.cpu().numpy().view(L.STATE_DTYPE)[:, 0], res.cpu().numpy().view(H.pkg().capi.limit_result_dtype())[:, 0]


def _against_model(out, rec, res, want, limiters, name=""):
    """every stream's output bytes, state bytes and result fields against its model, exactly (the two floats: one float32 step)"""
    for s, lim in enumerate(limiters):
        if out[s].tobytes() != want[s].tobytes():
            bad = np.argwhere(out[s] != want[s])
            raise AssertionError((name, s, "first difference at (instant, slot)", bad[0].tolist(), int(out[s][tuple(bad[0])]), int(want[s][tuple(bad[0])]), len(bad)))
        assert rec[s].tobytes() == lim.record().tobytes(), (name, s, rec[s], lim.record())
        rd, got = lim.read(), res[s]
        for k in ("samples", "reduced", "max_detect", "min_gain_q24", "flags"):
            assert int(got[k]) == rd[k], (name, s, k, int(got[k]), rd[k])
        assert np.all(got["reserved"] == 0), s
        for k in ("in_dbtp", "reduction_db"):
            assert abs(float(got[k]) - rd[k]) <= float(np.spacing(np.float32(abs(rd[k])))), (name, s, k, float(got[k]), rd[k])


def _check(engine, roles, C, R, pcm, name="", **kw):
    want, limiters = L.run_batch(pcm, roles, C, R)
    out, state, rec, res = _limit(engine, roles, C, R, pcm, **kw)
    _against_model(out, rec, res, want, limiters, name)
    return out, state, rec, res, limiters


def test_named_contents_against_the_model(engine):
    """the CPU test's named contents at -1 dBTP, R = 3496, each as one stream: output and state bytes are the model's"""
    for name, roles, pcm in L.contents():
        _, _, _, res, _ = _check(engine, roles, C1, R0, pcm[None], name)
        assert int(res["flags"][0]) == L.ACTIVE, name        # every one of them is over -1 dBTP somewhere


@pytest.mark.parametrize("streams", [1, 3, 4, 5, 70])
def test_stream_counts(engine, streams):
    """partial and multiple workgroups of four wavefronts; every stream gets different content and level"""
    pcm = np.stack([M.noise(500 + s, 2, 3, np.array((1.0, 0.8, 0.3)) * (1.0, 0.6, 0.3, 0.1)[s % 4]) for s in range(streams)])
    _, _, rec, _, _ = _check(engine, [1, 1, 0], C1, R0, pcm)
    assert len(rec) == streams and (streams < 4 or (rec["reduced"][0] > 0 and rec["reduced"][3] == 0))


def test_call_shapes_alignment_and_in_place(engine):
    """3 frames in one call = 1+2, 2+1 and 1+1+1; a 16-byte aligned base = base + 2 bytes; in place = out of place"""
    import torch
    pcm = np.stack([M.noise(600 + s, 3, 6, (1.0, 0.7, 0.5, 1.0, 0.3, 0.9), loud_slot=3) for s in range(5)])
    roles = [1, 1, 1, 0, 2, 2]
    out0, state0, _, res0, _ = _check(engine, roles, C1, R0, pcm)
    for cuts in ((3,), (1, 2), (2, 1), (1, 1, 1)):
        for offset in (0, 1):
            for in_place in (False, True):
                out, state, _, res = _limit(engine, roles, C1, R0, pcm, cuts=cuts, offset=offset, in_place=in_place)
                assert out.tobytes() == out0.tobytes() and torch.equal(state, state0) and res.tobytes() == res0.tobytes(), (cuts, offset, in_place)


def test_bursts_at_the_seams(engine):
    """one worst_case() burst whose last sample falls at index 22, 23, 24 (a lane seam), 76, 77, 78 (the delay), 1535, 1536,
    1537 (the frame seam, and with cuts (1, 2) the call seam) of a stream; and bursts at the end of lanes 0, 30, 59 and 63,
    whose hold reaches the next four lanes (or frame)"""
    ends = [22, 23, 24, 76, 77, 78, 1535, 1536, 1537] + [24 * k + 23 for k in (0, 30, 59, 63)] + [1536 + 24 * 62 + 23]
    pcm = np.zeros((len(ends), 3 * 1536, 2), np.int16)
    for s, end in enumerate(ends):
        first = max(end - 11, 0)
        pcm[s, first:end + 1, s % 2] = M.worst_case()[first - (end - 11):]
        pcm[s, :, 1 - s % 2] = 3000                     # a constant beside it: the gain is seen in the other slot's output
    for cuts in ((3,), (1, 2), (1, 1, 1)):
        for R in (R0, 1 << 20):
            out, _, rec, _, limiters = _check(engine, [1, 1], C1, R, pcm, cuts=cuts)
    g = L.limit(pcm[10], [1, 1], C1, 1 << 20)[1]        # the burst that ends lane 30: held over the 80 instants behind it
    assert np.all(g[24 * 31:24 * 31 + 4 * 24 - 16 - 64] < L.ONE) and rec[10]["reduced"] > 80


def test_release_ramp(engine):
    """a burst at the start, then silence: with R = 1 the gain is still recovering after three frames and two calls (the
    carried r), with R = 2^20 it is back at ONE sixteen samples after the hold"""
    pcm = np.zeros((2, 3 * 1536, 1), np.int16)
    pcm[:, 100:112, 0] = M.worst_case()
    pcm[1, 1536 + 700:1536 + 712, 0] = M.worst_case() // 2
    for R in (1, 1 << 20):
        out, _, rec, res, limiters = _check(engine, [1], C1, R, pcm, cuts=(1, 2))
        _check(engine, [1], C1, R, pcm, cuts=(3,))
        if R == 1:
            assert np.all(rec["r_red"][:, -1] > 0) and 3 * 1536 - 118 <= rec["reduced"][0] <= 3 * 1536 - 100
        else:
            assert np.all(rec["r_red"] == 0) and 80 <= rec["reduced"][0] < 200


@pytest.mark.parametrize("channels", [1, 2, 3, 4, 5, 6])
def test_channel_counts_and_roles(engine, channels):
    """1..6 channels, each with all slots detected and with a mask that leaves a full-scale slot undetected (from two
    channels on): that slot comes out delayed with the stream's gain and does not influence it; both load paths"""
    masks = [[1] * channels, [[1], [0, 2], [1, 0, 255], [0, 1, 1, 2], [1, 1, 0, 2, 2], [1, 0, 1, 0, 2, 1]][channels - 1]]
    for roles in masks:
        loud = roles.index(0) if 0 in roles else None
        pcm = np.stack([M.noise(7000 + 10 * channels + s, 2, channels, np.array((0.9, 0.5, 0.25, 1.0, 0.1, 0.7)) * (1.0, 0.8, 0.3)[s], loud_slot=loud)
                        for s in range(3)])
        out, state, rec, res, _ = _check(engine, roles, C1, R0, pcm)
        out1, state1, _, _ = _limit(engine, roles, C1, R0, pcm, offset=1)
        assert out1.tobytes() == out.tobytes() and state1.cpu().numpy().tobytes() == state.cpu().numpy().tobytes()
        if loud is not None:
            quiet = pcm.copy()
            quiet[:, :, loud] = 0
            out2, _, rec2, _ = _limit(engine, roles, C1, R0, quiet)
            keep = [c for c in range(channels) if c != loud]
            assert np.array_equal(out2[:, :, keep], out[:, :, keep]) and np.array_equal(rec2["r_red"], rec["r_red"])
            g = L.limit(pcm[0], roles, C1, R0)[1]
            x = pcm[0, :, loud].astype(np.int64)
            assert np.array_equal(out[0, 77:, loud], ((x[:-77] * g[77:] + (1 << 23)) >> 24).astype(np.int16))


def test_extremes(engine):
    """all -32768, all 32767 and silence in six channels, at C = 1, C = -1 dBTP and C = 2^28; a stream that never exceeds C
    comes out as its input delayed by 77, exactly, with `reduced` 0"""
    pcm = np.zeros((4, 2 * 1536, 6), np.int16)
    pcm[0], pcm[1] = -32768, 32767
    pcm[3] = M.noise(70, 2, 6, (0.4,) * 6)              # at most 0.4 * 16571 / 8192 = 0.81 of full scale: under -1 dBTP
    roles = [1, 1, 1, 0, 2, 2]
    for C in (1, C1, 1 << 28):
        out, _, rec, res, _ = _check(engine, roles, C, R0, pcm, cuts=(1, 1))
        assert not out[2].any() and rec["reduced"][2] == 0 and res["flags"][2] == 0
        if C == 1:
            assert not out[0, 200:].any() and res["min_gain_q24"][0] == 0
        else:
            assert np.array_equal(out[3, 77:], pcm[3, :-77]) and not out[3, :77].any() and rec["reduced"][3] == 0
            assert rec["reduced"][0] > 0 and np.abs(out[:2][:, :, (0, 1, 2, 4, 5)].astype(np.int64)).max() <= (C + 4096) >> 13


def test_read_kernel_against_the_host_twin(engine):
    """ac3mi_limit_read on the states the kernel left, and on a new stream's: byte-equal records"""
    import torch
    pkg = H.pkg()
    pcm = np.stack([M.noise(800 + s, 1, 2, np.array((1.0, 0.6)) * (1.0, 0.9, 0.1)[s]) for s in range(3)])     # sample peaks 1.0, 0.9, 0.1
    _, state, _, _ = _limit(engine, [1, 1], C2, R0, pcm)
    state = torch.cat([state, torch.zeros((1, NB), dtype=torch.uint8, device="cuda")])
    res = engine.limit_read_batch(state)
    engine.sync()
    raw, res = state.cpu().numpy(), res.cpu().numpy().view(pkg.capi.limit_result_dtype())[:, 0]
    for s in range(4):
        assert pkg.limit_read(raw[s].tobytes()).tobytes() == res[s].tobytes(), s
    assert res["flags"].tolist() == [L.ACTIVE, L.ACTIVE, 0, L.EMPTY] and res["in_dbtp"][3] == -200.0 and res["reduction_db"][3] == 0.0


def test_argument_errors_leave_state_and_output_alone(engine):
    import torch
    lib = engine.lib
    pcm = torch.zeros((1, 2, 1536, 6), dtype=torch.int16, device="cuda")
    out = torch.full((1, 2, 1536, 6), 0x5a5a, dtype=torch.int16, device="cuda")
    state = torch.full((1, NB), 0xa5, dtype=torch.uint8, device="cuda")
    role = (ctypes.c_uint8 * 6)(1, 1, 1, 0, 2, 2)
    torch.cuda.synchronize()

    def call(channels=6, roles=role, C=C1, R=R0, p=pcm.data_ptr(), o=out.data_ptr(), n=1, frames=2, st=state.data_ptr()):
        return lib.ac3mi_limit_batch(ctypes.c_void_p(engine.ctx), channels, roles, C, R, ctypes.c_void_p(p), ctypes.c_void_p(o), n, frames, ctypes.c_void_p(st))

    for kw in (dict(channels=0), dict(channels=7), dict(channels=-1), dict(roles=None), dict(p=None), dict(o=None), dict(st=None),
               dict(p=pcm.data_ptr() + 1), dict(o=out.data_ptr() + 1), dict(st=state.data_ptr() + 4), dict(frames=0), dict(frames=-3), dict(n=-1),
               dict(C=0), dict(C=(1 << 28) + 1), dict(R=0), dict(R=(1 << 20) + 1),
               dict(p=out.data_ptr() + 768 * 12, frames=1), dict(p=out.data_ptr(), o=out.data_ptr() + 2, frames=1)):     # partial overlaps
        assert call(**kw) == ERR_ARG, kw
        assert b"ac3mi_limit_batch" in lib.ac3mi_last_error(ctypes.c_void_p(engine.ctx))
    engine.sync()
    assert torch.equal(state, torch.full_like(state, 0xa5)) and torch.equal(out, torch.full_like(out, 0x5a5a))
    res = torch.zeros((1, 40), dtype=torch.uint8, device="cuda")
    assert lib.ac3mi_limit_read_batch(ctypes.c_void_p(engine.ctx), None, 1, ctypes.c_void_p(res.data_ptr())) == ERR_ARG
    assert lib.ac3mi_limit_read_batch(ctypes.c_void_p(engine.ctx), ctypes.c_void_p(state.data_ptr()), 1, ctypes.c_void_p(res.data_ptr() + 4)) == ERR_ARG
    assert call(n=0) == 0 and lib.ac3mi_limit_read_batch(ctypes.c_void_p(engine.ctx), ctypes.c_void_p(state.data_ptr()), 0, ctypes.c_void_p(res.data_ptr())) == 0
    engine.sync()
    assert torch.equal(state, torch.full_like(state, 0xa5)) and torch.equal(out, torch.full_like(out, 0x5a5a)) and int(res.sum()) == 0


def test_end_to_end_on_decoded_pcm(engine):
    """two hot 5.1 frames -> encode -> ac3mi_decode_s16_batch -> ac3mi_limit_batch at -2 dBTP -> ac3mi_truepeak_batch: the limited
    PCM is the model's, the meter's state on it is the true-peak model's on the model's output; the read-out's excess over C
    is printed, and the proved sample-peak bound asserted"""
    import torch
    pkg = H.pkg()
    S, F = 1, 2
    src = np.stack([M.noise(300, F, 6, (1.0, 1.0, 0.9, 0.8, 1.0, 0.9))])
    coded = T.encode(engine, src)
    fb = coded.shape[2]
    buf = np.zeros((S, F, (fb + 3) & ~3), np.uint8)
    buf[:, :, :fb] = coded
    dec = pkg.DecodeDesc(flags=7 | 16, level=1.0, bias=384.0, dynrng=1, acmod=7, lfeon=1, frame_bytes=fb)
    delay = torch.zeros((S, 6, 128), dtype=torch.float32, device="cuda")
    lfsr = torch.ones((S,), dtype=torch.int16, device="cuda")
    pcm16, status = engine.decode_s16_batch(dec, torch.from_numpy(buf).cuda(), delay, lfsr)
    engine.sync()
    assert int((status.cpu() & 0x1ff).max()) == 0
    pcm_dev = pcm16.view(S, F, 1536, 6)
    decoded = pcm_dev.cpu().numpy().reshape(S, F * 1536, 6)
    roles = pkg.loudness_roles(7 | 16)
    before = engine.truepeak_read_batch(engine.truepeak_batch(roles, pcm_dev), C2)
    out, state = engine.limit_batch(roles, C2, R0, pcm_dev)
    tp_state = engine.truepeak_batch(roles, out)
    after = engine.truepeak_read_batch(tp_state, C2)
    engine.sync()
    want, limiters = L.run_batch(decoded, roles, C2, R0)
    got = out.cpu().numpy().reshape(S, F * 1536, 6)
    assert got.tobytes() == want.tobytes() and state.cpu().numpy().view(L.STATE_DTYPE)[:, 0][0].tobytes() == limiters[0].record().tobytes()
    meters = M.run_batch(want, roles)
    assert tp_state.cpu().numpy().view(M.STATE_DTYPE)[:, 0][0].tobytes() == meters[0].record().tobytes()
    dt = pkg.capi.truepeak_result_dtype()
    before, after = before.cpu().numpy().view(dt)[:, 0][0], after.cpu().numpy().view(dt)[:, 0][0]
    print("decoded: %.3f dBTP (over: %d); limited at -2 dBTP: %.3f dBTP, true peak - C = %d (2^-28 of full scale)"
          % (before["dbtp"], before["flags"] & M.OVER, after["dbtp"], int(after["true_peak"]) - C2))
    assert before["flags"] & M.OVER and limiters[0].reduced > 0
    detected = [c for c in range(6) if roles[c]]
    assert int(np.abs(got[0][:, detected].astype(np.int64)).max()) <= (C2 + 4096) >> 13
