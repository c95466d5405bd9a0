"""GPU: loudness_kernel<.., RANGE> and loudness_range_read_kernel (ac3mi_loudness_range_batch, ac3mi_loudness_range_read_batch)
against tests/loudness_range_model.py - EBU Tech 3342 on the hop energies of the BS.1770 model, numpy float64 - on programmes
with a quiet lead-in that the relative gate removes and, in the quietest, the absolute one; the loudness state beside it
byte for byte what ac3mi_loudness_batch leaves; the device read-out byte for byte the host twin's; both states' independence
of how a stream is cut into calls and of the PCM's alignment."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _harness as H
from tests import loudness_model as M
from tests import loudness_range_content as C
from tests import loudness_range_model as R
from tests.test_loudness_gpu import ROLES6, _dev, _rel

pytestmark = pytest.mark.gpu

ERR_ARG = -1
TOL = 1e-9                              # energies: the loudness meter's tolerance (the hops are its hops)

_cache = {}


def _meter(engine, fs, roles, pcm, cuts=None, offset=0, states=(None, None)):
    """the engine's two meters over pcm [S][n][C] in calls of `cuts` frames (default: one call), each call's PCM `offset`
    int16 behind a 16-byte boundary -> (the loudness state tensor, the range state tensor, its records, the result records)"""
    state, rstate = states
    f = 0
    for n in cuts or (pcm.shape[1] // 1536,):
        state, rstate = engine.loudness_range_batch(fs, roles, _dev(pcm[:, 1536 * f:1536 * (f + n)], offset), state, rstate)
        f += n
    assert 1536 * f == pcm.shape[1]
    res = engine.loudness_range_read_batch(rstate)
    engine.sync()
    return (state, rstate, rstate.cpu().numpy().view(R.RANGE_STATE_DTYPE)[:, 0],
            res.cpu().numpy().view(H.pkg().capi.loudness_range_result_dtype())[:, 0])


def _main_on_device(engine, fs):
    if fs not in _cache:
        _cache[fs] = _meter(engine, fs, ROLES6, C.main()[fs][0])
    return _cache[fs]


def _against_model(rec, res, meters):
    """every stream's range state and result against its meter -> the largest relative difference of any energy"""
    worst = 0.0
    for s, m in enumerate(meters):
        st, got, want = rec[s], res[s], m.range_read()
        assert np.array_equal(st["count"], m.r_count), s
        assert (int(st["hops"]), int(st["ring_pos"]), int(st["blocks"]), int(st["blocks_abs"])) == (m.r_hops, m.ring_pos, m.r_blocks, m.r_blocks_abs), s
        d = max(_rel(st["ring"], m.ring), _rel(st["sum_abs"], m.sum_abs), _rel(st["max_short"], m.max_short),
                _rel(got["max_short_energy"], m.max_short))
        worst = max(worst, d)
        assert d <= TOL, (s, d)
        for k in ("blocks", "blocks_abs", "blocks_rel", "lra_tenths", "low_bin", "high_bin", "flags"):
            assert int(got[k]) == int(want[k]), (s, k, got[k], want[k])
        assert np.all(got["reserved"] == 0), s
        # the floats are those of the integers
        assert got["lra"].tobytes() == (np.float32(0.1) * np.float32(int(got["lra_tenths"]))).tobytes(), s
        if int(got["flags"]) & R.EMPTY:
            assert float(got["low_lkfs"]) == float(got["high_lkfs"]) == -70.0 and int(got["lra_tenths"]) == int(got["low_bin"]) == int(got["high_bin"]) == 0, s
        else:
            assert got["low_lkfs"].tobytes() == R.bin_lkfs(got["low_bin"]).tobytes() and got["high_lkfs"].tobytes() == R.bin_lkfs(got["high_bin"]).tobytes(), s
        ms = float(R.max_short_lkfs(float(got["max_short_energy"])))
        assert abs(float(got["max_short_lkfs"]) - ms) <= 2.0 ** -23 * abs(ms), s
    return worst


@pytest.mark.parametrize("fs", M.RATES)
def test_against_the_model(engine, fs):
    """9 streams x 320 frames x 6 channels in one call: bins, counters, ring position, lra_tenths, both bins and flags equal,
    ring, sum_abs and max_short to 1e-9"""
    _, _, rec, res = _main_on_device(engine, fs)
    worst = _against_model(rec, res, C.main()[fs][1])
    print("%d Hz: largest relative difference of any energy from the float64 model %.3g; lra_tenths %s" % (fs, worst, res["lra_tenths"].tolist()))
    assert len(set(res["lra_tenths"].tolist())) >= 3 and np.all(res["blocks_rel"] > 0)


@pytest.mark.parametrize("fs", M.RATES)
def test_the_loudness_state_is_the_plain_meters(engine, fs):
    """the loudness state that ac3mi_loudness_range_batch leaves is byte for byte the one ac3mi_loudness_batch leaves on the
    same PCM: six channels (the main content) and 1, 2, 3 and 5, from either alignment"""
    import torch
    state = _main_on_device(engine, fs)[0]
    plain = engine.loudness_batch(fs, ROLES6, _dev(C.main()[fs][0]))
    engine.sync()
    assert torch.equal(state, plain)
    for flags in C.CHANNEL_FLAGS:
        _, roles, pcm, _ = C.channels(flags)
        for offset in (0, 1):
            plain = engine.loudness_batch(fs, roles, _dev(pcm, offset))
            both = engine.loudness_range_batch(fs, roles, _dev(pcm, offset))[0]
            engine.sync()
            assert torch.equal(both, plain), (flags, offset)


def test_read_kernel_equals_the_host_twin(engine):
    """ac3mi_loudness_range_read on the states the kernel left: the device's 48-byte records byte for byte"""
    pkg = H.pkg()
    for fs in M.RATES:
        _, rstate, _, res = _main_on_device(engine, fs)
        raw = rstate.cpu().numpy()
        for s in range(C.S_MAIN):
            assert pkg.loudness_range_read(raw[s].tobytes()).tobytes() == res[s].tobytes(), (fs, s)


def test_call_shapes_and_alignment_leave_the_same_bits(engine):
    """44.1 kHz (the hop boundary falls inside a lane's segment): one call of 320 frames, 320 calls of one, 16 + 304, and the
    one call again from a base 2 bytes off a 16-byte boundary (the 16-bit loads) - identical bytes in both states and
    identical results; with the unmeasured LFE slot zeroed, identical again; with a measured slot zeroed, not"""
    import torch
    fs = 44100
    pcm = C.main()[fs][0]
    one, rone, _, res_one = _main_on_device(engine, fs)
    for name, kw in (("320 x 1", dict(cuts=(1,) * 320)), ("16 + 304", dict(cuts=(16, 304))), ("2 bytes off", dict(offset=1))):
        st, rst, _, res = _meter(engine, fs, ROLES6, pcm, **kw)
        assert torch.equal(st, one) and torch.equal(rst, rone), name
        assert res.tobytes() == res_one.tobytes(), name
    quiet_lfe = pcm.copy()
    quiet_lfe[:, :, 3] = 0
    st, rst, _, res = _meter(engine, fs, ROLES6, quiet_lfe)
    assert torch.equal(st, one) and torch.equal(rst, rone) and res.tobytes() == res_one.tobytes()
    other = pcm.copy()
    other[:, :, 4] = 0
    assert not torch.equal(_meter(engine, fs, ROLES6, other)[1], rone)


@pytest.mark.parametrize("flags", C.CHANNEL_FLAGS)
def test_channel_counts(engine, flags):
    """1, 2, 3 and 5 channels with the roles of their s16 layouts, 4 streams x 128 frames at 32 kHz, both load paths"""
    import torch
    fs, roles, pcm, meters = C.channels(flags)
    assert H.pkg().loudness_roles(flags) == roles and all(m.r_blocks == 128 * 1536 // 3200 - 29 for m in meters)
    st, rst, rec, res = _meter(engine, fs, roles, pcm)
    print("%d channels at %d Hz: %.3g, lra_tenths %s" % (len(roles), fs, _against_model(rec, res, meters), res["lra_tenths"].tolist()))
    st2, rst2, _, res2 = _meter(engine, fs, roles, pcm, offset=1)
    assert torch.equal(st2, st) and torch.equal(rst2, rst) and res2.tobytes() == res.tobytes()


def test_tech_3342_case_on_the_device(engine):
    """Tech 3342's -40 / -30 case: a 1 kHz stereo sine at 32 kHz, 20 s at each level, its first 833 whole frames in one call:
    lra_tenths within 100 +- 10, and the model's where scipy filters the 1.28 million samples"""
    pcm = R.r128_sine((-40, -30))[:833 * 1536][None]
    _, _, rec, res = _meter(engine, 32000, [1, 1], pcm)
    print("lra_tenths %d, %d blocks, %d counted" % (res["lra_tenths"][0], res["blocks"][0], res["blocks_rel"][0]))
    assert abs(int(res["lra_tenths"][0]) - 100) <= 10 and int(res["blocks"][0]) == 833 * 1536 // 3200 - 29 and int(res["flags"][0]) == 0
    if R.HAVE_LFILTER:
        meters = R.run_batch(pcm, 32000, [1, 1])
        assert meters[0].range_margin() > 1e-6
        _against_model(rec, res, meters)


def test_extremes(engine):
    """digital silence; full-scale square waves on all six slots; a first call shorter than 3 s, continued"""
    import torch
    fs, F = 48000, 128                                  # 40 hops: 11 blocks
    silence = np.zeros((2, F * 1536, 6), np.int16)
    _, _, rec, res = _meter(engine, fs, ROLES6, silence)
    want = R.run_batch(silence, fs, ROLES6)
    assert want[0].r_blocks == 11 and np.all(rec["blocks"] == 11) and np.all(rec["count"] == 0) and np.all(rec["blocks_abs"] == 0)
    assert np.all(rec["sum_abs"] == 0) and np.all(rec["max_short"] == 0) and np.all(rec["hops"] == 40) and np.all(rec["ring_pos"] == 10)
    assert np.all(res["flags"] == R.EMPTY) and np.all(res["blocks"] == 11) and np.all(res["blocks_rel"] == 0) and np.all(res["lra_tenths"] == 0)
    assert np.all(res["low_lkfs"] == -70.0) and np.all(res["high_lkfs"] == -70.0) and np.all(res["max_short_lkfs"] == -200.0)
    _against_model(rec, res, want)
    square = np.where((np.arange(F * 1536) // 24) % 2 == 0, 32767, -32768).astype(np.int16)[None, :, None].repeat(6, axis=2)
    _, _, rec_sq, res_sq = _meter(engine, fs, ROLES6, square)
    _against_model(rec_sq, res_sq, R.run_batch(square, fs, ROLES6))
    assert np.isfinite(res_sq["max_short_energy"][0]) and np.isfinite(res_sq["max_short_lkfs"][0]) and res_sq["max_short_lkfs"][0] > 0
    assert res_sq["flags"][0] == 0 and res_sq["low_bin"][0] > 700 and res_sq["lra_tenths"][0] == 0 and res_sq["blocks_rel"][0] == 11
    # 16 frames are half a second: no block yet; the states go on into the next call as if the stream had not been cut
    pcm = np.stack([M.programme(190 + s, F, 6, 0.2, quiet_part=0.3, loud_slot=3) for s in range(2)])
    st1, rst1, rec1, res1 = _meter(engine, fs, ROLES6, pcm[:, :16 * 1536])
    assert np.all(rec1["hops"] == 5) and np.all(rec1["ring_pos"] == 5) and np.all(rec1["blocks"] == 0) and np.all(rec1["ring"][:, :5] > 0)
    assert np.all(rec1["ring"][:, 5:] == 0) and np.all(res1["flags"] == R.EMPTY)
    st2, rst2, rec2, res2 = _meter(engine, fs, ROLES6, pcm[:, 16 * 1536:], states=(st1, rst1))
    whole, rwhole, _, res_whole = _meter(engine, fs, ROLES6, pcm)
    assert torch.equal(st2, whole) and torch.equal(rst2, rwhole) and res2.tobytes() == res_whole.tobytes()
    _against_model(rec2, res2, R.run_batch(pcm, fs, ROLES6))


def test_argument_errors_leave_both_states_alone(engine):
    import torch
    pkg = H.pkg()
    lib = engine.lib
    pcm = torch.zeros((1, 1, 1536, 6), dtype=torch.int16, device="cuda")
    state = torch.full((1, pkg.loudness_state_bytes()), 0xa5, dtype=torch.uint8, device="cuda")
    rstate = torch.full((1, pkg.loudness_range_state_bytes()), 0xa5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def call(rate=48000, channels=6, roles=ROLES6, p=pcm.data_ptr(), st=state.data_ptr(), rst=rstate.data_ptr(), n=1, frames=1):
        desc = pkg.capi.LoudnessDescC(rate, channels, (ctypes.c_uint8 * 6)(*roles))
        return lib.ac3mi_loudness_range_batch(ctypes.c_void_p(engine.ctx), ctypes.byref(desc), ctypes.c_void_p(p), n, frames,
                                              ctypes.c_void_p(st), ctypes.c_void_p(rst))

    for kw in (dict(rate=24000), dict(rate=22050), dict(rate=11025), dict(rate=0), dict(rate=96000), dict(channels=0), dict(channels=7),
               dict(channels=-1), dict(roles=[1, 1, 3, 0, 2, 2]), dict(roles=[255, 1, 1, 0, 2, 2]), dict(p=None), dict(st=None),
               dict(rst=None), dict(p=pcm.data_ptr() + 1), dict(st=state.data_ptr() + 4), dict(rst=rstate.data_ptr() + 4),
               dict(rst=rstate.data_ptr() + 1), dict(frames=0), dict(n=-1)):
        assert call(**kw) == ERR_ARG, kw
        assert b"ac3mi_loudness_range_batch" in lib.ac3mi_last_error(ctypes.c_void_p(engine.ctx))
    res = torch.zeros((1, 48), dtype=torch.uint8, device="cuda")
    for st, out in ((None, res.data_ptr()), (rstate.data_ptr(), None), (rstate.data_ptr() + 4, res.data_ptr()), (rstate.data_ptr(), res.data_ptr() + 4)):
        assert lib.ac3mi_loudness_range_read_batch(ctypes.c_void_p(engine.ctx), ctypes.c_void_p(st), 1, ctypes.c_void_p(out)) == ERR_ARG
        assert b"ac3mi_loudness_range_read_batch" in lib.ac3mi_last_error(ctypes.c_void_p(engine.ctx))
    assert lib.ac3mi_loudness_range_read_batch(ctypes.c_void_p(engine.ctx), ctypes.c_void_p(rstate.data_ptr()), -1, ctypes.c_void_p(res.data_ptr())) == ERR_ARG
    assert call(n=0) == 0
    assert lib.ac3mi_loudness_range_read_batch(ctypes.c_void_p(engine.ctx), ctypes.c_void_p(rstate.data_ptr()), 0, ctypes.c_void_p(res.data_ptr())) == 0
    engine.sync()
    assert torch.equal(state, torch.full_like(state, 0xa5)) and torch.equal(rstate, torch.full_like(rstate, 0xa5))
    assert torch.equal(res, torch.zeros_like(res))


def test_timing_script_runs():
    """profiles/loudness_range_ab.py on a small batch: it runs, the range pass leaves the plain meter's loudness state and
    its two load paths the same range state (its own assertions) and it prints one parseable JSON line (no timing is
    asserted)"""
    r = subprocess.run([sys.executable, os.path.join(H.ROOT, "profiles", "loudness_range_ab.py"), "--streams", "256", "--passes", "2"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().split("\n")[-1])
    assert res["streams"] == 256 and res["pcm_bytes"] == 256 * 1536 * 6 * 2
    for case in ("loudness_batch", "loudness_batch_unaligned", "loudness_range_batch", "loudness_range_batch_unaligned", "loudness_read_batch", "loudness_range_read_batch"):
        assert res[case]["median_ms"] > 0 and res[case]["passes"] == 2
    assert res["range_over_plain"] > 0
