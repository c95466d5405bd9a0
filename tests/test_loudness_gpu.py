"""GPU: loudness_kernel, loudness_read_kernel and loudness_words_kernel (ac3mi_loudness_batch, ac3mi_loudness_read_batch,
ac3mi_loudness_words_batch) against tests/loudness_model.py - the BS.1770 meter run sample by sample in numpy float64 - on
programmes whose quiet part the relative gate removes, at the three rates; the state's independence of how a stream is cut
into calls and of the PCM's alignment; then end to end: decoded PCM -> meter -> dialnorm words -> encoder."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _harness as H
from tests import _tools as T
from tests import loudness_model as M

pytestmark = pytest.mark.gpu

ERR_ARG = -1
S_MAIN, F_MAIN = 9, 64                  # nine wavefronts: more than two workgroups of four
ROLES6 = [1, 1, 1, 0, 2, 2]             # WAVE order FL FR FC LFE BL BR
AMPS = (1.0, 0.6, 0.35, 0.2, 0.1, 0.05, 0.025, 0.012, 0.006)    # the dialnorms from the clamp at 1 to the clamp at 31
SEEDS = {48000: 4800, 44100: 4410, 32000: 3200}
MARGIN = 1e-6                           # no decision of the content may hang on less than this (relative)
TOL = 1e-9                              # energies: four orders above what the segmented filter differs from the recursion

_cache = {}


def _main():
    """the main content and its model, once: rate -> (pcm int16 [9][64 * 1536][6], the nine meters); the LFE slot is loud
    and not measured"""
    if "main" not in _cache:
        pcm = {fs: np.stack([M.programme(SEEDS[fs] + s, F_MAIN, 6, AMPS[s], loud_slot=3) for s in range(S_MAIN)]) for fs in M.RATES}
        meters = M.run_batch(np.concatenate([pcm[fs] for fs in M.RATES]), [fs for fs in M.RATES for _ in range(S_MAIN)], ROLES6)
        _cache["main"] = {fs: (pcm[fs], meters[S_MAIN * i:S_MAIN * (i + 1)]) for i, fs in enumerate(M.RATES)}
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


def _meter(engine, fs, roles, pcm, cuts=None, offset=0, state=None):
    """the engine's meter over pcm [S][n][C] in calls of `cuts` frames (default: one call), each call's PCM `offset` int16
    behind a 16-byte boundary -> (the state tensor, its records, the result records)"""
    f = 0
    for n in cuts or (pcm.shape[1] // 1536,):
        state = engine.loudness_batch(fs, roles, _dev(pcm[:, 1536 * f:1536 * (f + n)], offset), state)
        f += n
    assert 1536 * f == pcm.shape[1]
    res = engine.loudness_read_batch(state)
    engine.sync()
    return state, state.cpu().numpy().view(M.STATE_DTYPE)[:, 0], res.cpu().numpy().view(H.pkg().capi.loudness_result_dtype())[:, 0]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nz = b != 0
    assert np.all(a[~nz] == 0)
    return float(np.max(np.abs(a[nz] / b[nz] - 1.0))) if nz.any() else 0.0


def _against_model(rec, res, meters, roles):
    """every stream's state and result against its meter -> the largest relative difference of any energy"""
    worst = 0.0
    for s, m in enumerate(meters):
        want = m.read()
        st = rec[s]
        assert np.array_equal(st["count"], m.count), s
        assert (int(st["pos"]), int(st["hop_count"]), int(st["blocks"]), int(st["blocks_abs"])) == (m.pos, m.hop_count, m.blocks, m.blocks_abs), s
        d = max(_rel(st["sum"], m.sum), _rel(st["hop_sum"], m.hop_sum), _rel(st["hops"], m.hops), _rel(st["max_block"], m.max_block),
                _rel(res[s]["max_block_energy"], m.max_block), _rel(res[s]["mean_energy"], want["mean_energy"]))
        worst = max(worst, d)
        assert d <= TOL, (s, d)
        for c, role in enumerate(roles):
            if role:
                assert np.allclose(st["bq"][c], m.bq[c], rtol=0, atol=1e-9), (s, c)
            else:
                assert np.all(st["bq"][c] == 0), (s, c)
        assert np.all(st["bq"][len(roles):] == 0)
        got = res[s]
        assert (int(got["blocks"]), int(got["blocks_abs"]), int(got["blocks_rel"])) == (m.blocks, m.blocks_abs, want["blocks_rel"]), s
        assert int(got["dialnorm"]) == want["dialnorm"] and int(got["flags"]) == want["flags"] and np.all(got["reserved"] == 0), s
        assert abs(float(got["lkfs"]) - want["lkfs"]) <= 1e-4, s
    return worst


def test_content_decides_nothing_on_a_rounding():
    """(the model alone) no block energy within 1e-6 relative of a bin edge, the absolute gate or the relative gate, no mean
    within 1e-6 of a dialnorm threshold; the relative gate removes blocks in every stream; three or more dialnorms occur,
    both clamps among them"""
    for fs, (pcm, meters) in _main().items():
        assert [m.blocks for m in meters] == [F_MAIN * 1536 // (fs // 10) - 3] * S_MAIN and meters[0].blocks == {48000: 17, 44100: 19, 32000: 27}[fs]
        margin = min(m.margin() for m in meters)
        reads = [m.read() for m in meters]
        dn = [r["dialnorm"] for r in reads]
        print("%d Hz: margin %.3g, dialnorms %s, blocks removed by the relative gate %s" %
              (fs, margin, dn, [r["blocks_abs"] - r["blocks_rel"] for r in reads]))
        assert margin > MARGIN
        assert all(r["blocks_abs"] > r["blocks_rel"] > 0 for r in reads)
        assert len(set(dn)) >= 3 and 1 in dn and 31 in dn


@pytest.mark.parametrize("fs", M.RATES)
def test_against_the_model(engine, fs):
    """9 streams x 64 frames x 6 channels in one call: bins, counters, dialnorm and flags equal, energies to 1e-9"""
    pcm, meters = _main()[fs]
    state, rec, res = _meter(engine, fs, ROLES6, pcm)
    worst = _against_model(rec, res, meters, ROLES6)
    print("%d Hz: largest relative difference of any energy from the float64 recursion %.3g" % (fs, worst))
    _cache[("state", fs)] = (state, rec, res)


def test_read_kernel_against_the_host_twin(engine):
    """ac3mi_loudness_read on the states the kernel left: the same counts, dialnorm and flags, mean_energy to 1e-12 (the
    lanes sum the bins in another order than the host), lkfs to one float32 step"""
    pkg = H.pkg()
    for fs in M.RATES:
        if ("state", fs) not in _cache:
            pcm, _ = _main()[fs]
            _cache[("state", fs)] = _meter(engine, fs, ROLES6, pcm)
        state, rec, res = _cache[("state", fs)]
        raw = state.cpu().numpy()
        for s in range(S_MAIN):
            host = pkg.loudness_read(raw[s].tobytes())
            for k in ("blocks", "blocks_abs", "blocks_rel", "dialnorm", "flags"):
                assert int(host[k]) == int(res[s][k]), (fs, s, k)
            assert float(host["max_block_energy"]) == float(res[s]["max_block_energy"])
            assert abs(float(host["mean_energy"]) / float(res[s]["mean_energy"]) - 1.0) <= 1e-12
            assert abs(float(host["lkfs"]) - float(res[s]["lkfs"])) <= 4e-6


def test_call_shapes_and_alignment_leave_the_same_bits(engine):
    """44.1 kHz (the hop boundary falls inside a lane's segment): one call of 64 frames, 64 calls of one, 16 + 48, and the
    one call again from a base 2 bytes off a 16-byte boundary (the 16-bit loads) - identical state bytes and results; with
    the unmeasured LFE slot zeroed, identical again"""
    import torch
    fs = 44100
    pcm, _ = _main()[fs]
    one, _, res_one = _meter(engine, fs, ROLES6, pcm)
    for name, kw in (("64 x 1", dict(cuts=(1,) * 64)), ("16 + 48", dict(cuts=(16, 48))), ("2 bytes off", dict(offset=1)),
                     ("2 bytes off, 16 + 48", dict(offset=1, cuts=(16, 48)))):
        st, _, res = _meter(engine, fs, ROLES6, pcm, **kw)
        assert torch.equal(st, one), name
        assert res.tobytes() == res_one.tobytes(), name
    quiet_lfe = pcm.copy()
    quiet_lfe[:, :, 3] = 0
    st, _, res = _meter(engine, fs, ROLES6, quiet_lfe)
    assert torch.equal(st, one) and res.tobytes() == res_one.tobytes()
    # ... and the measured slots do matter
    other = pcm.copy()
    other[:, :, 4] = 0
    assert not torch.equal(_meter(engine, fs, ROLES6, other)[0], one)


@pytest.mark.parametrize("flags,fs", [(1, 48000), (2, 44100), (3, 32000), (7, 44100)])
def test_channel_counts(engine, flags, fs):
    """1, 2, 3 and 5 channels with the roles of their s16 layouts, 4 streams x 16 frames, both load paths"""
    import torch
    roles = H.pkg().loudness_roles(flags)
    C = len(roles)
    assert C == {1: 1, 2: 2, 3: 3, 7: 5}[flags]
    pcm = np.stack([M.programme(7000 + 10 * C + s, 16, C, (0.8, 0.3, 0.1, 0.03)[s], quiet_part=0.3) for s in range(4)])
    meters = M.run_batch(pcm, fs, roles)
    assert min(m.margin() for m in meters) > MARGIN and all(m.blocks == 16 * 1536 // (fs // 10) - 3 for m in meters)
    state, rec, res = _meter(engine, fs, roles, pcm)
    print("%d channels at %d Hz: %.3g" % (C, fs, _against_model(rec, res, meters, roles)))
    assert torch.equal(_meter(engine, fs, roles, pcm, offset=1)[0], state)


def test_extremes(engine):
    """digital silence; full-scale square waves on all six slots; a first call of one frame, continued"""
    import torch
    pkg = H.pkg()
    fs = 48000
    silence = np.zeros((2, 16 * 1536, 6), np.int16)
    _, rec, res = _meter(engine, fs, ROLES6, silence)
    assert np.all(rec["count"] == 0) and np.all(rec["sum"] == 0) and np.all(rec["blocks"] == 2) and np.all(rec["blocks_abs"] == 0)
    assert np.all(res["flags"] == M.EMPTY) and np.all(res["dialnorm"] == 31) and np.all(res["mean_energy"] == 0) and np.all(res["blocks_rel"] == 0)
    # an empty stream keeps the base word's dialnorm, a measured one gets its own
    base = pkg.encode_metadata_word(dialnorm=27, bsmod=2)
    square = np.where((np.arange(16 * 1536) // 24) % 2 == 0, 32767, -32768).astype(np.int16)[None, :, None].repeat(6, axis=2)
    meters = M.run_batch(square, fs, ROLES6)
    _, rec_sq, res_sq = _meter(engine, fs, ROLES6, square)
    _against_model(rec_sq, res_sq, meters, ROLES6)
    assert np.isfinite(res_sq["mean_energy"][0]) and res_sq["dialnorm"][0] == 1 and res_sq["flags"][0] == 0 and res_sq["lkfs"][0] > 0
    assert rec_sq["count"][0].sum() == 2 and np.nonzero(rec_sq["count"][0])[0].min() > 700
    both = torch.from_numpy(np.stack([res.view(np.uint8).reshape(-1, 40)[0], res_sq.view(np.uint8).reshape(-1, 40)[0]])).cuda()
    words = engine.loudness_words_batch(both, 3, base)
    engine.sync()
    assert words.cpu().numpy().view(np.uint32).tolist() == [[base] * 3, [(base & ~31) | 1] * 3]
    # one frame only: no hop has closed; the state goes on into the next call as if the stream had not been cut
    pcm = np.stack([M.programme(90 + s, 16, 6, 0.2, quiet_part=0.0, loud_slot=3) for s in range(2)])
    st1, rec1, res1 = _meter(engine, fs, ROLES6, pcm[:, :1536])
    assert np.all(rec1["pos"] == 1536) and np.all(rec1["hop_count"] == 0) and np.all(rec1["blocks"] == 0) and np.all(rec1["hop_sum"] > 0)
    assert np.all(res1["flags"] == M.EMPTY) and np.all(res1["dialnorm"] == 31)
    st2, rec2, res2 = _meter(engine, fs, ROLES6, pcm[:, 1536:], state=st1)
    whole, _, res_whole = _meter(engine, fs, ROLES6, pcm)
    assert torch.equal(st2, whole) and res2.tobytes() == res_whole.tobytes()
    _against_model(rec2, res2, M.run_batch(pcm, fs, ROLES6), ROLES6)


def test_argument_errors_leave_the_state_alone(engine):
    import torch
    pkg = H.pkg()
    lib = engine.lib
    pcm = torch.zeros((1, 1, 1536, 6), dtype=torch.int16, device="cuda")
    state = torch.full((1, pkg.loudness_state_bytes()), 0xa5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def call(rate=48000, channels=6, roles=ROLES6, p=pcm.data_ptr(), st=state.data_ptr(), n=1, frames=1):
        desc = pkg.capi.LoudnessDescC(rate, channels, (ctypes.c_uint8 * 6)(*roles))
        return lib.ac3mi_loudness_batch(ctypes.c_void_p(engine.ctx), ctypes.byref(desc), ctypes.c_void_p(p), n, frames, ctypes.c_void_p(st))

    for kw in (dict(rate=24000), dict(rate=22050), dict(rate=11025), dict(rate=0), dict(rate=96000), dict(channels=0), dict(channels=7),
               dict(channels=-1), dict(roles=[1, 1, 3, 0, 2, 2]), dict(roles=[255, 1, 1, 0, 2, 2]), dict(p=None), dict(st=None),
               dict(p=pcm.data_ptr() + 1), dict(st=state.data_ptr() + 4), dict(frames=0), dict(n=-1)):
        assert call(**kw) == ERR_ARG, kw
        assert b"ac3mi_loudness_batch" in lib.ac3mi_last_error(ctypes.c_void_p(engine.ctx))
    engine.sync()
    assert torch.equal(state, torch.full_like(state, 0xa5))
    res = torch.zeros((1, 40), dtype=torch.uint8, device="cuda")
    assert lib.ac3mi_loudness_read_batch(ctypes.c_void_p(engine.ctx), None, 1, ctypes.c_void_p(res.data_ptr())) == ERR_ARG
    assert lib.ac3mi_loudness_words_batch(ctypes.c_void_p(engine.ctx), ctypes.c_void_p(res.data_ptr()), 1, 0, 0, ctypes.c_void_p(res.data_ptr())) == ERR_ARG
    assert call(n=0) == 0 and lib.ac3mi_loudness_read_batch(ctypes.c_void_p(engine.ctx), ctypes.c_void_p(state.data_ptr()), 0, ctypes.c_void_p(res.data_ptr())) == 0


def test_end_to_end_dialnorm_into_the_encoder(engine):
    """two 2/0 programmes 20 dB apart, 16 frames: coded, decoded to s16 on the device, metered there, read, turned into
    words, and coded again under those words - every new frame carries the model's dialnorm for its programme, the two are
    20 apart, and with the words taken away the encoder is back at its default bytes"""
    import torch
    pkg = H.pkg()
    F = 16
    loud = M.programme(321, F, 2, 0.5, quiet_part=0.0)
    src = np.stack([loud, np.round(loud * 0.1).astype(np.int16)])
    coded = T.encode(engine, src)
    S, _, fb = coded.shape
    buf = np.zeros((S, F, (fb + 3) & ~3), np.uint8)
    buf[:, :, :fb] = coded
    dec = pkg.DecodeDesc(flags=2, level=1.0, bias=384.0, dynrng=1, acmod=2, lfeon=0, frame_bytes=fb)
    delay = torch.zeros((S, 2, 128), dtype=torch.float32, device="cuda")
    lfsr = torch.ones((S,), dtype=torch.int16, device="cuda")
    pcm16, status = engine.decode_s16_batch(dec, torch.from_numpy(buf).cuda(), delay, lfsr)
    engine.sync()
    assert int((status.cpu() & 0x1ff).max()) == 0
    pcm_dev = pcm16.view(S, F, 1536, 2)
    roles = pkg.loudness_roles(2)
    state = engine.loudness_batch(48000, roles, pcm_dev)
    results = engine.loudness_read_batch(state)
    base = pkg.encode_metadata_word(bsmod=1)
    words = engine.loudness_words_batch(results, F, base)
    engine.sync()
    decoded = pcm_dev.cpu().numpy().reshape(S, F * 1536, 2)
    meters = M.run_batch(decoded, 48000, roles)
    assert min(m.margin() for m in meters) > MARGIN
    want = [m.read()["dialnorm"] for m in meters]
    res = results.cpu().numpy().view(pkg.capi.loudness_result_dtype())[:, 0]
    print("dialnorms %s, %.3f and %.3f LKFS" % (want, res["lkfs"][0], res["lkfs"][1]))
    assert res["dialnorm"].tolist() == want and 19 <= want[1] - want[0] <= 21 and 1 < want[0] and want[1] < 31
    try:
        default = T.encode(engine, decoded)
        engine.set_encode_metadata_frames(words)
        got = T.encode(engine, decoded)
        for s in range(S):
            for f in range(F):
                fields, _ = T.bsi_view(got[s, f])
                assert fields["dialnorm"] == want[s] and fields["bsmod"] == 1, (s, f, fields)
        engine.set_encode_metadata_frames(None)
        assert np.array_equal(T.encode(engine, decoded), default)
    finally:
        engine.set_encode_metadata_frames(None)


def test_timing_script_runs():
    """profiles/loudness_ab.py on a small batch: it runs, its two load paths leave the same state (its own assertion) and it
    prints one parseable JSON line (no timing is asserted)"""
    r = subprocess.run([sys.executable, os.path.join(H.ROOT, "profiles", "loudness_ab.py"), "--streams", "256", "--passes", "2"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().split("\n")[-1])
    assert res["streams"] == 256 and res["pcm_bytes"] == 256 * 1536 * 6 * 2
    for case in ("loudness_batch", "loudness_batch_unaligned", "loudness_read_batch", "loudness_words_batch", "encode_drc0", "encode_drc1"):
        assert res[case]["median_ms"] > 0 and res[case]["passes"] == 2
