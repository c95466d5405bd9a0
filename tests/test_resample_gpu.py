"""GPU: resample_kernel (ac3mi_resample_batch) against tests/resample_model.py - the converter's rule in numpy int64 - byte for
byte: the output PCM, the state and d_status; their independence of how a stream is cut into calls, of the buffers' alignment
and of what the workspaces held; the refusals, which leave a stream untouched; the host twin; then end to end between the
project's own decoder and encoder."""
import ctypes

import numpy as np
import pytest

from tests import _harness as H
from tests import _tools as T
from tests import resample_model as R

pytestmark = pytest.mark.gpu

ERR_ARG = -1
NB = R.STATE_DTYPE.itemsize
UP, DOWN = (44100, 48000), (48000, 44100)


def _dev(pcm, offset=0):
    """int16 [S][n][C] -> a device tensor [S][F][1536][C] whose base lies `offset` int16 behind a 16-byte boundary"""
    import torch
    S, n, C = pcm.shape
    flat = torch.zeros(pcm.size + 8, dtype=torch.int16, device="cuda")
    assert flat.data_ptr() % 16 == 0
    t = flat[offset:offset + pcm.size]
    t.copy_(torch.from_numpy(np.ascontiguousarray(pcm).reshape(-1)))
    return t.view(S, n // 1536, 1536, C)


def _convert(engine, pair, pcm, cuts=None, offset=0, state=None, age=(0, 0)):
    """the engine's converter over pcm [S][n][C] in calls of `cuts` frames (default: one call), each with the out_frames planned
    for streams of `age` (samples_in, frames_out), each call's buffers `offset` int16 behind a 16-byte boundary ->
    (out int16 [S][m][C], the state tensor, its records, the statuses of every call [calls][S], the out_frames of every call)"""
    S, _, C = pcm.shape
    f, outs, stats, taken = 0, [], [], []
    n_in, f_out = age
    for n in cuts or (pcm.shape[1] // 1536,):
        of, _ = R.plan(*pair, n_in, f_out, n)
        x = _dev(pcm[:, 1536 * f:1536 * (f + n)], offset)
        out = _dev(np.full((S, 1536 * of, C), 0x5a5a, np.int16), offset)
        out, state, status = engine.resample_batch(pair, x, of, state, out)
        outs.append(out)
        stats.append(status)
        taken.append(of)
        f += n
        n_in += 1536 * n
        f_out += of
    assert 1536 * f == pcm.shape[1]
    engine.sync()
    out = np.concatenate([o.cpu().numpy().reshape(S, -1, C) for o in outs], axis=1)
    return out, state, state.cpu().numpy().view(R.STATE_DTYPE)[:, 0], np.stack([s.cpu().numpy() for s in stats]), taken


def _against_model(out, rec, want, convs, name=""):
    for s, conv in enumerate(convs):
        if out[s].tobytes() != want[s].tobytes():
            bad = np.argwhere(out[s] != want[s])
            raise AssertionError((name, s, "first difference at (instant, slot)", bad[0].tolist(), int(out[s][tuple(bad[0])]),
                                  int(want[s][tuple(bad[0])]), len(bad)))
        assert rec[s].tobytes() == conv.record().tobytes(), (name, s)


def _check(engine, pair, pcm, name="", **kw):
    want, convs = R.run_batch(*pair, pcm)
    out, state, rec, status, taken = _convert(engine, pair, pcm, **kw)
    assert not status.any(), (name, status)
    _against_model(out, rec, want, convs, name)
    return out, state, rec, taken


def test_named_contents_and_cuts(engine):
    """the named contents at 44.1 -> 48 kHz in six channels, three streams a batch: twelve one-frame calls, of which the twelfth
    takes two frames, and one twelve-frame call that takes thirteen"""
    import torch
    named = R.contents(44100, 12, 6)
    named.append(("noise again", R.contents(44100, 12, 6, seed=1)[2][1]))
    for batch in (named[:3], named[3:]):
        pcm = np.stack([x for _, x in batch])
        names = [k for k, _ in batch]
        _, state1, _, taken = _check(engine, UP, pcm, names, cuts=(1,) * 12)
        assert taken == [1] * 11 + [2]
        out, state2, rec, taken = _check(engine, UP, pcm, names)
        assert taken == [13] and torch.equal(state1, state2) and int(rec["samples_in"][0]) == 12 * 1536 and int(rec["frames_out"][0]) == 13
        if "full-scale random" in names:
            assert (out == -32768).any() and (out == 32767).any()


@pytest.mark.parametrize("pair,cuts", [(UP, (1, 2)), (DOWN, (1, 2)), ((32000, 48000), (1, 1)), ((48000, 32000), (1, 3)),
                                       ((32000, 44100), (1, 1, 1)), ((44100, 32000), (1, 2))])
def test_pairs(engine, pair, cuts):
    """all six pairs, two channels, four streams, through calls that take no frame (the decimating pairs' first) and two"""
    pcm = np.stack([R.contents(pair[0], sum(cuts), 2, seed=10 + s)[1 + s % 3][1] for s in range(4)])
    _, _, _, taken = _check(engine, pair, pcm, pair, cuts=cuts)
    assert 2 in taken and (pair[0] < pair[1] or taken[0] == 0), taken
    _check(engine, pair, pcm, pair)


@pytest.mark.parametrize("streams", [1, 3, 4, 5, 70])
def test_stream_counts(engine, streams):
    pcm = np.stack([R.contents(44100, 2, 2, seed=100 + s)[2][1] for s in range(streams)])
    _, _, rec, _ = _check(engine, UP, pcm, streams, cuts=(1, 1))
    assert len(rec) == streams


@pytest.mark.parametrize("channels", [1, 2, 3, 4, 5, 6])
def test_channel_counts(engine, channels):
    """the longest filter (96 taps) and the largest table (441 phases)"""
    for pair, cuts in (((48000, 32000), (1, 2)), ((32000, 44100), (2,))):
        pcm = np.stack([R.contents(pair[0], sum(cuts), channels, seed=200 + s)[2 + s][1] for s in range(2)])
        _check(engine, pair, pcm, (pair, channels), cuts=cuts)


def test_alignment(engine):
    """d_pcm and d_out one sample behind a 16-byte boundary: the same bits as aligned; and with 3 and 5 channels (5 streams x
    2 frames), where an instant's slots straddle the 16-byte boundaries differently"""
    import torch
    pcm = np.stack([R.contents(44100, 3, 6, seed=300 + s)[2][1] for s in range(3)])
    out0, state0, _, _ = _check(engine, UP, pcm, cuts=(1, 2))
    out1, state1, _, _ = _check(engine, UP, pcm, cuts=(1, 2), offset=1)
    assert out0.tobytes() == out1.tobytes() and torch.equal(state0, state1)
    for channels in (3, 5):
        pcm = np.stack([R.contents(44100, 2, channels, seed=310 + s)[2][1] for s in range(5)])
        out0, state0, _, _ = _check(engine, UP, pcm, channels)
        out1, state1, _, _ = _check(engine, UP, pcm, channels, offset=1)
        assert out0.tobytes() == out1.tobytes() and torch.equal(state0, state1), channels


def test_extremes(engine):
    """+- full-scale random input in every pair's direction: the sum leaves an s16 on both sides and is clamped at both rails"""
    for pair in (UP, (48000, 32000)):
        pcm = np.stack([R.contents(pair[0], 3, 2, seed=400 + s)[3][1] for s in range(2)])
        out, _, _, _ = _check(engine, pair, pcm, pair)
        assert (out == -32768).any() and (out == 32767).any()


def test_mixed_ages(engine):
    """32 -> 48 kHz: a new stream's first frame gives one frame, a stream's second gives two.  Streams 1 and 3 are a frame older
    than the rest; the call asks for one frame: they get status 1, their state stays byte for byte and their frame is zeros,
    and the others are converted as if they were alone"""
    import torch
    pair = (32000, 48000)
    pcm = np.stack([R.contents(32000, 2, 2, seed=500 + s)[2][1] for s in range(5)])
    old = [1, 3]
    state = torch.zeros((5, NB), dtype=torch.uint8, device="cuda")
    _, sub, _, status, taken = _convert(engine, pair, pcm[old, :1536])
    assert taken == [1] and not status.any()
    state[old] = sub
    before = state.cpu().numpy().copy()
    out, state, rec, status, taken = _convert(engine, pair, pcm[:, 1536:], state=state)
    assert taken == [1] and status[0].tolist() == [0, R.STATUS_FRAMES, 0, R.STATUS_FRAMES, 0]
    after = state.cpu().numpy()
    new = [0, 2, 4]
    assert np.array_equal(after[old], before[old]) and not out[old].any()
    want, convs = R.run_batch(*pair, pcm[new, 1536:])
    _against_model(out[new], rec[new], want, convs)
    # asked for their own two frames, the older streams go on as if nothing had happened
    out2, state, status = engine.resample_batch(pair, _dev(pcm[:, 1536:]), 2, state)
    engine.sync()
    assert not status.cpu().numpy().any()
    want, convs = R.run_batch(*pair, pcm[old])
    got = out2.cpu().numpy().reshape(5, -1, 2)
    assert got[old].tobytes() == want[:, 1536:].tobytes()
    rec = state.cpu().numpy().view(R.STATE_DTYPE)[:, 0]
    assert all(rec[s].tobytes() == c.record().tobytes() for s, c in zip(old, convs))


def test_pair_mismatch(engine):
    """a state started at 44.1 -> 48 kHz in two channels, then called the other way round or with three channels: status 2, the
    state byte for byte, zeros for output; a new stream beside it in the same call is converted"""
    import torch
    pcm = np.stack([R.contents(44100, 1, 2, seed=600 + s)[2][1] for s in range(2)])
    _, state, _, _ = _check(engine, UP, pcm[:1])
    state = torch.cat([state, torch.zeros((1, NB), dtype=torch.uint8, device="cuda")])
    before = state.cpu().numpy().copy()
    for pair, ch in ((DOWN, 2), (UP, 3)):
        x = np.stack([R.contents(pair[0], 1, ch, seed=610 + s)[2][1] for s in range(2)])
        of, _ = R.plan(*pair, 0, 0, 1)
        out = _dev(np.full((2, 1536 * max(of, 1), ch), 0x5a5a, np.int16))[:, :of].contiguous()
        st = state.clone()
        out, st, status = engine.resample_batch(pair, _dev(x), of, st, out)
        engine.sync()
        assert status.cpu().numpy().tolist() == [R.STATUS_STATE, 0], (pair, ch)
        assert np.array_equal(st.cpu().numpy()[0], before[0]) and not out.cpu().numpy()[0].any()
        want, convs = R.run_batch(*pair, x[1:])
        assert out.cpu().numpy()[1].tobytes() == want[0].tobytes() and st.cpu().numpy()[1].tobytes() == convs[0].record().tobytes()


def test_argument_errors_leave_state_and_output_alone(engine):
    import torch
    lib = engine.lib
    pkg = H.pkg()
    pcm = torch.zeros((1, 2, 1536, 6), dtype=torch.int16, device="cuda")
    out = torch.full((1, 2, 1536, 6), 0x5a5a, dtype=torch.int16, device="cuda")
    state = torch.full((1, NB), 0xa5, dtype=torch.uint8, device="cuda")
    status = torch.full((1,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def call(rates=UP, ch=6, desc=True, p=pcm.data_ptr(), n=1, fin=2, o=out.data_ptr(), fout=2, st=state.data_ptr(), ds=status.data_ptr()):
        d = pkg.ResampleDesc(rates[0], rates[1], ch)
        return lib.ac3mi_resample_batch(ctypes.c_void_p(engine.ctx), ctypes.byref(d) if desc else None, ctypes.c_void_p(p), n, fin,
                                        ctypes.c_void_p(o), fout, ctypes.c_void_p(st), ctypes.c_void_p(ds))

    for kw in (dict(rates=(24000, 48000)), dict(rates=(44100, 22050)), dict(rates=(0, 48000)), dict(rates=(48000, 48000)), dict(rates=(44100, 44100)),
               dict(ch=0), dict(ch=7), dict(ch=-1), dict(desc=False), dict(fin=0), dict(fin=-1), dict(fout=-1), dict(n=-1),
               dict(p=None), dict(o=None), dict(st=None), dict(ds=None), dict(p=pcm.data_ptr() + 1), dict(o=out.data_ptr() + 1),
               dict(st=state.data_ptr() + 4), dict(ds=status.data_ptr() + 2),
               dict(p=out.data_ptr()), dict(p=out.data_ptr() + 768 * 12, fin=1), dict(p=out.data_ptr() - 3072 * 6 + 2, fin=1)):     # overlaps
        assert call(**kw) == ERR_ARG, kw
        assert b"ac3mi_resample_batch" in lib.ac3mi_last_error(ctypes.c_void_p(engine.ctx))
    assert lib.ac3mi_resample_batch(None, None, None, 0, 0, None, 0, None, None) == ERR_ARG
    assert call(n=0) == 0
    engine.sync()
    assert torch.equal(state, torch.full_like(state, 0xa5)) and torch.equal(out, torch.full_like(out, 0x5a5a))
    assert int(status[0]) == 0x5a5a5a5a


def test_host_twin_gives_the_device_bytes(engine):
    """ac3mi_resample_host on one stream, call by call beside the device: output, state and status"""
    pkg = H.pkg()
    for pair, ch in ((UP, 6), ((44100, 32000), 3)):
        pcm = R.contents(pair[0], 3, ch, seed=700)[2][1]
        out, _, rec, _, taken = _convert(engine, pair, pcm[None], cuts=(1, 2))
        st, outs = None, []
        for f, n, of in ((0, 1, taken[0]), (1, 2, taken[1])):
            o, st, status = pkg.resample_host(pair, pcm[1536 * f:1536 * (f + n)], of, st)
            assert status == 0
            outs.append(o)
        assert np.concatenate(outs).tobytes() == out[0].tobytes() and st == rec[0].tobytes(), (pair, ch)


def test_workspaces_do_not_matter(engine):
    import torch
    pcm = np.stack([R.contents(44100, 2, 6, seed=800 + s)[2][1] for s in range(3)])
    got = []
    for byte in (0x00, 0xa5):
        engine.fill_workspaces(byte)
        out, state, _, _ = _check(engine, UP, pcm, byte, cuts=(1, 1))
        got.append((out, state))
    assert got[0][0].tobytes() == got[1][0].tobytes() and torch.equal(got[0][1], got[1][1])


def test_end_to_end_441_to_48(engine):
    """a 2/0 programme at 44.1 kHz - a 997 Hz tone - coded by the project's encoder -> ac3mi_decode_s16_batch ->
    ac3mi_resample_batch (44.1 -> 48, planned) -> ac3mi_encode_batch at 48 kHz: every frame passes both CRCs, its BSI says
    fscod 0, and decoded again the tone is at 997 Hz, not at 997 * 48 / 44.1 = 1085 Hz where re-labelling would put it"""
    import torch
    pkg = H.pkg()
    S, F = 1, 12
    src = R.tone(997.0, 44100, F * 1536, 2, amp=12000.0)[None]
    coded = T.encode(engine, src, sr=44100, rate=192000)
    fb = coded.shape[2]
    buf = np.zeros((S, F, (fb + 3) & ~3), np.uint8)
    buf[:, :, :fb] = coded
    dec = pkg.DecodeDesc(flags=2, level=1.0, bias=384.0, dynrng=1, acmod=2, lfeon=0, frame_bytes=fb)
    delay = torch.zeros((S, 2, 128), dtype=torch.float32, device="cuda")
    lfsr = torch.ones((S,), dtype=torch.int16, device="cuda")
    pcm16, status = engine.decode_s16_batch(dec, torch.from_numpy(buf).cuda(), delay, lfsr)
    engine.sync()
    assert int((status.cpu() & 0x1ff).max()) == 0
    pcm_dev = pcm16.view(S, F, 1536, 2)
    of, left = pkg.resample_plan(44100, 48000, 0, 0, F)
    assert (of, left) == (13, 95)
    out, state, rstatus = engine.resample_batch(UP, pcm_dev, of)
    engine.sync()
    assert not rstatus.cpu().numpy().any()
    decoded = pcm_dev.cpu().numpy().reshape(S, F * 1536, 2)
    want, convs = R.run_batch(44100, 48000, decoded)
    got = out.cpu().numpy().reshape(S, of * 1536, 2)
    assert got.tobytes() == want.tobytes() and state.cpu().numpy().view(R.STATE_DTYPE)[0, 0].tobytes() == convs[0].record().tobytes()
    again = T.encode(engine, got, sr=48000, rate=192000)
    assert again.shape[:2] == (S, of)
    fb2 = again.shape[2]
    buf2 = np.zeros((S, of, (fb2 + 3) & ~3), np.uint8)
    buf2[:, :, :fb2] = again
    verdict = engine.crc_check_batch(torch.from_numpy(buf2).cuda(), fb2)
    engine.sync()
    assert not verdict.cpu().numpy().any()
    for f in range(of):
        assert int(pkg.bsi_read(again[0, f])["fscod"]) == 0 and pkg.syncinfo(again[0, f])[2] == 48000
    pcm2, st2, _ = T.decode(engine, again, 2, 0)
    assert (st2 & 0x1ff).max() == 0
    y = pcm2[0, :, :, 0, :].reshape(-1)[2 * 1536:]          # slot 0 behind the rise
    spec = np.abs(np.fft.rfft(y * np.hanning(len(y))))
    hz = 48000.0 / len(y)
    peak = int(np.argmax(spec)) * hz
    assert abs(peak - 997.0) <= hz and abs(peak - 997.0 * 48000 / 44100) > 10 * hz, (peak, hz)
