"""GPU: truepeak_kernel and truepeak_read_kernel (ac3mi_truepeak_batch, ac3mi_truepeak_read_batch) against
tests/truepeak_model.py - BS.1770-4 Annex 2's interpolator in numpy int64 - bit for bit: the state bytes and every integer
of the result; the state's independence of how a stream is cut into calls and of the PCM's alignment; peaks whose maximum
lies in the next lane, frame or call; then end to end on decoded PCM."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _harness as H
from tests import _tools as T
from tests import truepeak_model as M

pytestmark = pytest.mark.gpu

ERR_ARG = -1
S_MAIN, F_MAIN = 9, 5                   # nine wavefronts: more than two workgroups of four
ROLES6 = [1, 1, 1, 0, 2, 2]             # WAVE order FL FR FC LFE BL BR
AMPS6 = (0.9, 0.5, 0.25, 1.0, 0.1, 0.7)

_cache = {}


def _main():
    """the main content and its model, once: (pcm int16 [9][5 * 1536][6], the nine meters); the levels differ by slot and
    stream, the LFE slot is loud and not measured"""
    if "main" not in _cache:
        pcm = np.stack([M.noise(900 + s, F_MAIN, 6, np.array(AMPS6) * (1.0, 0.7, 0.4, 0.2, 0.1, 0.05, 0.02, 0.01, 0.001)[s], loud_slot=3)
                        for s in range(S_MAIN)])
        _cache["main"] = (pcm, M.run_batch(pcm, ROLES6))
    return _cache["main"]


def _dev(pcm, offset=0):
    """int16 [S][n][C] -> a device tensor [S][F][1536][C] whose base lies `offset` int16 behind a 16-byte boundary"""
    import torch
    S, n, C = pcm.shape
    flat = torch.zeros(pcm.size + 8, dtype=torch.int16, device="cuda")
    assert flat.data_ptr() % 16 == 0
    t = flat[offset:offset + pcm.size]
    t.copy_(torch.from_numpy(np.ascontiguousarray(pcm).reshape(-1)))
    return t.view(S, n // 1536, 1536, C)


def _meter(engine, roles, pcm, cuts=None, offset=0, state=None, ceiling=0):
    """the engine's meter over pcm [S][n][C] in calls of `cuts` frames (default: one call), each call's PCM `offset` int16
    behind a 16-byte boundary -> (the state tensor, its records, the result records)"""
    f = 0
    for n in cuts or (pcm.shape[1] // 1536,):
        state = engine.truepeak_batch(roles, _dev(pcm[:, 1536 * f:1536 * (f + n)], offset), state)
        f += n
    assert 1536 * f == pcm.shape[1]
    res = engine.truepeak_read_batch(state, ceiling)
    engine.sync()
    return state, state.cpu().numpy().view(M.STATE_DTYPE)[:, 0], res.cpu().numpy().view(H.pkg().capi.truepeak_result_dtype())[:, 0]


def _against_model(rec, res, meters, ceiling=0):
    """every stream's state bytes and result fields against its meter, exactly (dbtp and dbfs: one float32 step)"""
    for s, m in enumerate(meters):
        assert rec[s].tobytes() == m.record().tobytes(), (s, rec[s], m.record())
        want, got = m.read(ceiling), res[s]
        for k in ("true_peak", "true_peak_index", "true_peak_slot", "sample_peak", "sample_peak_slot", "full_scale", "samples", "flags"):
            assert int(got[k]) == want[k], (s, k, int(got[k]), want[k])
        assert got["slot_true_peak"].tolist() == want["slot_true_peak"] and got["slot_sample_peak"].tolist() == want["slot_sample_peak"], s
        assert np.all(got["reserved"] == 0), s
        for k in ("dbtp", "dbfs"):
            assert abs(float(got[k]) - want[k]) <= float(np.spacing(np.float32(abs(want[k])))), (s, k, float(got[k]), want[k])


def test_against_the_model(engine):
    """9 streams x 5 frames x 6 channels in one call: state bytes and result fields equal the model's"""
    pcm, meters = _main()
    state, rec, res = _meter(engine, ROLES6, pcm)
    _against_model(rec, res, meters)
    assert np.all(rec["true_peak"][:, 3] == 0) and np.all(rec["hist"][:, 3] == 0) and np.all(rec["measured"] == 0b110111)
    assert np.all(res["true_peak"] > res["sample_peak"].astype(np.int64) << 13)
    _cache["state"] = (state, rec, res)


def test_call_shapes_and_alignment_leave_the_same_bits(engine):
    """the same PCM cut as (5), (1, 4), (4, 1) and (1, 1, 1, 1, 1), at int16 offsets 0, 1 and 3 behind a 16-byte boundary
    (offsets 1 and 3: the 16-bit loads): identical state bytes and results"""
    import torch
    pcm, _ = _main()
    one, _, res_one = _meter(engine, ROLES6, pcm)
    for cuts in ((5,), (1, 4), (4, 1), (1, 1, 1, 1, 1)):
        for offset in (0, 1, 3):
            st, _, res = _meter(engine, ROLES6, pcm, cuts=cuts, offset=offset)
            assert torch.equal(st, one), (cuts, offset)
            assert res.tobytes() == res_one.tobytes(), (cuts, offset)
    # the unmeasured slot does not matter, the measured ones do
    other = pcm.copy()
    other[:, :, 3] = 0
    assert torch.equal(_meter(engine, ROLES6, other)[0], one)
    other = pcm.copy()
    other[:, :, 4] = 0
    assert not torch.equal(_meter(engine, ROLES6, other)[0], one)


def test_boundary_peaks(engine):
    """one isolated full-scale sample at the last instant of a frame inside a call, at the last instant of a call, at
    instants 23 and 24 of a frame (a lane boundary) and at instant 0 of the stream: the maximum (7964 times the sample, first
    in phase 3 five instants on, again in phase 0 six on) lies in the next lane, frame or call - value and index are the
    model's.  A wrong history hand-off fails here."""
    F = 4
    places = {"last of a frame inside a call": 1535, "last of a call": 2 * 1536 - 1, "instant 23": 3 * 1536 + 23, "instant 24": 3 * 1536 + 24,
              "instant 0 of the stream": 0, "eleven before a frame's end": 1536 - 11, "lane 62 / 63": 1536 + 63 * 24 - 1}
    pcm = np.zeros((len(places), F * 1536, 2), np.int16)
    for s, at in enumerate(places.values()):
        pcm[s, at, s % 2] = (32767, -32768)[s % 2]
    meters = M.run_batch(pcm, [1, 1])
    for s, (name, at) in enumerate(places.items()):
        m = meters[s]
        assert m.true_peak[s % 2] == 7964 * (32767, 32768)[s % 2] and m.index[s % 2] == 4 * (at + 5) + 3 and m.full_scale[s % 2] == 1, name
    for cuts in ((2, 2), (4,), (1, 1, 1, 1)):
        for offset in (0, 1):
            _, rec, res = _meter(engine, [1, 1], pcm, cuts=cuts, offset=offset)
            _against_model(rec, res, meters)
    # ... and with the sample as a call's very last, the maximum exists only once the next call has come
    st, rec, _ = _meter(engine, [1, 1], pcm[1:2, :2 * 1536])
    head = M.run_batch(pcm[1:2, :2 * 1536], [1, 1])
    assert rec[0].tobytes() == head[0].record().tobytes() and head[0].true_peak[1] < meters[1].true_peak[1]
    _, rec, res = _meter(engine, [1, 1], pcm[1:2, 2 * 1536:], state=st)
    _against_model(rec, res, meters[1:2])


@pytest.mark.parametrize("channels", [1, 2, 3, 4, 5, 6])
def test_channel_counts_and_roles(engine, channels):
    """1..6 channels with mixed roles (an unmeasured loud slot from three channels on; role 255 measures), 5 streams x 3
    frames and x 1 frame, both load paths"""
    import torch
    roles = [[1], [2, 1], [1, 0, 255], [0, 1, 1, 2], [1, 1, 0, 2, 2], [1, 0, 1, 0, 2, 1]][channels - 1]
    loud = roles.index(0) if 0 in roles else None
    for F in (3, 1):
        pcm = np.stack([M.noise(7000 + 10 * channels + s + F, F, channels, np.array(AMPS6) * (1.0, 0.5, 0.2, 0.05, 0.01)[s], loud_slot=loud) for s in range(5)])
        meters = M.run_batch(pcm, roles)
        state, rec, res = _meter(engine, roles, pcm)
        _against_model(rec, res, meters)
        assert torch.equal(_meter(engine, roles, pcm, offset=1)[0], state)


def test_extremes(engine):
    """the worst-case pattern across a frame boundary, all -32768, digital silence, in six channels: the model's bits, the
    largest |y| the table allows, full_scale counted"""
    pcm = np.zeros((3, 2 * 1536, 6), np.int16)
    pcm[0, 1536 - 5:1536 + 7, 4] = M.worst_case()
    pcm[0, 100:112, 3] = M.worst_case()                 # (the unmeasured slot)
    pcm[1] = -32768
    meters = M.run_batch(pcm, ROLES6)
    assert meters[0].true_peak[4] == 32768 * 12271 + 32767 * 4300 and meters[0].full_scale == [0, 0, 0, 0, 12, 0]
    assert meters[1].full_scale == [3072, 3072, 3072, 0, 3072, 3072] and meters[1].sample_peak[0] == 32768
    assert meters[2].true_peak == [0] * 6 and meters[2].index == [0] * 6
    for cuts in ((2,), (1, 1)):
        _, rec, res = _meter(engine, ROLES6, pcm, cuts=cuts, ceiling=M.ceiling(-1))
        _against_model(rec, res, meters, ceiling=M.ceiling(-1))
        assert res["flags"].tolist() == [M.OVER, M.OVER, 0] and res["full_scale"].tolist() == [12, 5 * 3072, 0]
        assert res["dbtp"][2] == -200.0 and res["dbfs"][2] == -200.0 and res["dbtp"][0] > 6.0


def test_ties(engine):
    """two identical bursts in one stream: the index is the first one's; the same burst in two slots: the lower slot's"""
    shape = np.array([900, -12000, 32767, -32768, 15000, -700], np.int16)
    pcm = np.zeros((2, 3 * 1536, 3), np.int16)
    for at in (700, 1536 + 1530):
        pcm[0, at:at + 6, 1] = shape
    pcm[1, 2000:2006, 2] = shape
    pcm[1, 2000:2006, 1] = shape
    meters = M.run_batch(pcm, [1, 1, 1])
    assert 4 * 700 <= meters[0].index[1] < 4 * 720 and meters[1].index[1] == meters[1].index[2] and meters[1].true_peak[1] == meters[1].true_peak[2]
    for cuts in ((3,), (1, 2), (2, 1)):
        _, rec, res = _meter(engine, [1, 1, 1], pcm, cuts=cuts)
        _against_model(rec, res, meters)
        assert res["true_peak_slot"].tolist() == [1, 1] and res["sample_peak_slot"].tolist() == [1, 1]


def test_read_kernel_against_the_host_twin(engine):
    """ac3mi_truepeak_read on the states the kernel left: byte-equal records, with and without a ceiling"""
    pkg = H.pkg()
    if "state" not in _cache:
        _cache["state"] = _meter(engine, ROLES6, _main()[0])
    state, rec, res0 = _cache["state"]
    raw = state.cpu().numpy()
    ceiling = int(np.sort(res0["true_peak"])[S_MAIN // 2])          # over for some streams, not for others
    res1 = engine.truepeak_read_batch(state, ceiling)
    engine.sync()
    res1 = res1.cpu().numpy().view(pkg.capi.truepeak_result_dtype())[:, 0]
    for s in range(S_MAIN):
        assert pkg.truepeak_read(raw[s].tobytes(), 0).tobytes() == res0[s].tobytes(), s
        assert pkg.truepeak_read(raw[s].tobytes(), ceiling).tobytes() == res1[s].tobytes(), s
    over = (res1["flags"] & M.OVER) != 0
    assert 0 < over.sum() < S_MAIN and np.array_equal(over, res0["true_peak"] > ceiling) and np.all(res0["flags"] == 0)


def test_argument_errors_leave_the_state_alone(engine):
    import torch
    pkg = H.pkg()
    lib = engine.lib
    pcm = torch.zeros((1, 1, 1536, 6), dtype=torch.int16, device="cuda")
    state = torch.full((1, pkg.truepeak_state_bytes()), 0xa5, dtype=torch.uint8, device="cuda")
    role = (ctypes.c_uint8 * 6)(*ROLES6)
    torch.cuda.synchronize()

    def call(channels=6, roles=role, p=pcm.data_ptr(), st=state.data_ptr(), n=1, frames=1):
        return lib.ac3mi_truepeak_batch(ctypes.c_void_p(engine.ctx), channels, roles, ctypes.c_void_p(p), n, frames, ctypes.c_void_p(st))

    for kw in (dict(channels=0), dict(channels=7), dict(channels=-1), dict(roles=None), dict(p=None), dict(st=None), dict(p=pcm.data_ptr() + 1),
               dict(st=state.data_ptr() + 4), dict(frames=0), dict(frames=-3), dict(n=-1)):
        assert call(**kw) == ERR_ARG, kw
        assert b"ac3mi_truepeak_batch" in lib.ac3mi_last_error(ctypes.c_void_p(engine.ctx))
    engine.sync()
    assert torch.equal(state, torch.full_like(state, 0xa5))
    res = torch.zeros((1, 96), dtype=torch.uint8, device="cuda")
    assert lib.ac3mi_truepeak_read_batch(ctypes.c_void_p(engine.ctx), None, 1, 0, ctypes.c_void_p(res.data_ptr())) == ERR_ARG
    assert lib.ac3mi_truepeak_read_batch(ctypes.c_void_p(engine.ctx), ctypes.c_void_p(state.data_ptr()), 1, 0, ctypes.c_void_p(res.data_ptr() + 4)) == ERR_ARG
    assert call(n=0) == 0 and lib.ac3mi_truepeak_read_batch(ctypes.c_void_p(engine.ctx), ctypes.c_void_p(state.data_ptr()), 0, 0, ctypes.c_void_p(res.data_ptr())) == 0
    engine.sync()
    assert torch.equal(state, torch.full_like(state, 0xa5)) and int(res.sum()) == 0


def test_end_to_end_on_decoded_pcm(engine):
    """nine encoded 5.1 frames (three streams of three) -> ac3mi_decode_s16_batch -> ac3mi_truepeak_batch on its output, with
    the roles ac3mi_loudness_roles gives = the model on the same s16; the loudness meter takes the same PCM beside it"""
    import torch
    pkg = H.pkg()
    S, F = 3, 3
    src = np.stack([M.noise(300 + s, F, 6, np.array(AMPS6) * (1.0, 0.3, 0.05)[s]) for s in range(S)])
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
    roles = pkg.loudness_roles(7 | 16)
    assert roles == ROLES6
    state = engine.truepeak_batch(roles, pcm_dev)
    loud = engine.loudness_batch(48000, roles, pcm_dev)
    res = engine.truepeak_read_batch(state, M.ceiling(-1))
    engine.sync()
    decoded = pcm_dev.cpu().numpy().reshape(S, F * 1536, 6)
    meters = M.run_batch(decoded, roles)
    _against_model(state.cpu().numpy().view(M.STATE_DTYPE)[:, 0], res.cpu().numpy().view(pkg.capi.truepeak_result_dtype())[:, 0], meters, M.ceiling(-1))
    assert meters[0].true_peak[0] > meters[2].true_peak[0] > 0 and int(loud.cpu().numpy().view(np.uint8).max()) > 0


def test_timing_script_runs():
    """profiles/truepeak_ab.py on a small batch: it runs, its two load paths leave the same state (its own assertion) and it
    prints one parseable JSON line (no timing is asserted)"""
    r = subprocess.run([sys.executable, os.path.join(H.ROOT, "profiles", "truepeak_ab.py"), "--streams", "256", "--passes", "2"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().split("\n")[-1])
    assert res["streams"] == 256 and res["pcm_bytes"] == 256 * 1536 * 6 * 2
    for case in ("truepeak_batch", "truepeak_batch_unaligned", "truepeak_read_batch", "loudness_batch"):
        assert res[case]["median_ms"] > 0 and res[case]["passes"] == 2
    assert res["copy_probe_ms_for_pcm_bytes"] > 0
