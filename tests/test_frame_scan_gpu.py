"""GPU: frame_scan_kernel and frame_gather_kernel (ac3mi_frame_scan_batch, ac3mi_frame_gather_batch) against
tests/frame_scan_model.py - the reference's resync rule on many dirty byte streams at once, with and without CRC-confirmed
sync - then end to end: bytes -> scan -> gather -> ac3mi_decode_s16_batch against the same frames laid out by the host, and
against the byte-stream layer's own host loop."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _harness as H
from tests import frame_scan_model as M

pytestmark = pytest.mark.gpu

STRIDE = 16384
MAX_FRAMES = 12
POOL = ((0, 0), (0, 4), (0, 8), (0, 14), (1, 20), (1, 21), (2, 0), (0, 28), (2, 37))      # 128 .. 3840 bytes

_cache = {}


def _random_stream(rng, target):
    """elements drawn from the CPU tests' cases until `target` bytes are there, cut to exactly that"""
    parts, n = [], 0
    while n < target:
        kind = rng.choice(["g", "g", "f", "f", "f", "f", "c", "p", "b", "h", "G"])
        fscod, code = POOL[int(rng.integers(0, len(POOL) - (2 if target < 6000 else 0)))]
        fr = M.frame(fscod, code, int(rng.integers(0, 2)))
        if kind == "g":
            x = M.garbage(int(rng.integers(1, 60)), int(rng.integers(0, 1 << 30)))
        elif kind == "G":                                   # more than one round of the cooperative search
            x = M.garbage(int(rng.integers(900, 2400)), int(rng.integers(0, 1 << 30)))
        elif kind == "f":
            x = fr
        elif kind == "c":
            x = fr[:int(rng.integers(8, len(fr)))]
        elif kind == "p":                                   # a valid header in garbage
            x = M.garbage(int(rng.integers(8, 200)), int(rng.integers(0, 1 << 30)))
            x[:8] = M.header(fscod, code)
        elif kind == "b":                                   # one flipped bit in either CRC region
            x = fr
            x[int(rng.integers(8, len(fr)))] ^= np.uint8(1 << int(rng.integers(0, 8)))
        else:                                               # a sync word with nothing behind it
            x = M.garbage(int(rng.integers(2, 30)), int(rng.integers(0, 1 << 30)))
            x[:2] = (0x0b, 0x77)
        parts.append(x)
        n += len(x)
    return np.concatenate(parts)[:target] if parts else np.zeros(0, np.uint8)


def _streams():
    """64 streams of at most 16 KiB: the named cases first, seeded random mixes behind them -> (list of byte arrays, and per
    mode the model's (frames, info) of every stream at MAX_FRAMES)"""
    if "streams" not in _cache:
        rng = np.random.default_rng(6464)
        fr = lambda k, seed=0: M.frame(*POOL[k], seed)       # noqa: E731
        s = [np.zeros(0, np.uint8),                                                     # empty
             M.garbage(5000, 1),                                                        # only garbage
             fr(2)[:7], fr(2)[:8],
             M.dirty_stream()[0],
             np.concatenate([fr(8), fr(7), M.garbage(13, 2), fr(8, 1), fr(7, 1)]),      # 3840- and 1536-byte frames mixed
             np.concatenate([fr(4 + (i & 1), i & 1) for i in range(6)] + [M.garbage(9, 3)]),     # the 44.1 kHz pair
             np.concatenate([x for i in range(8) for x in (M.garbage(1 + (i == 4), 40 + i), fr(0, i & 1))]),   # every byte alignment
             np.concatenate([fr(0, i & 1) for i in range(30)]),                          # more frames than MAX_FRAMES
             np.concatenate([M.garbage(3000, 4), fr(3), M.garbage(2500, 5), fr(3, 1)]),  # searches of several rounds
             np.concatenate([fr(7), fr(7, 1)] * 5 + [M.garbage(STRIDE - 10 * 1536, 6)]),   # len == stride
             np.concatenate([M.garbage(STRIDE - 1536 - 8, 7), fr(7), fr(7)[:8]]),        # a frame that ends 8 bytes before the stride, a header in the last 8 bytes
             M.garbage(STRIDE, 8)]
        assert len(s[10]) == STRIDE and len(s[11]) == STRIDE
        while len(s) < 64:
            s.append(_random_stream(rng, int(rng.integers(0, STRIDE + 1))))
        _cache["streams"] = s
        _cache["want"] = {mode: [M.scan(x, mode, MAX_FRAMES) for x in s] for mode in (0, 1)}
        flags = [w[1]["flags"] for w in _cache["want"][1]]
        assert M.CAPPED in flags and M.INCOMPLETE in flags and sum(w[1]["rejected"] for w in _cache["want"][1]) > 20
        assert _cache["want"][0] != _cache["want"][1]
    return _cache["streams"], _cache["want"]


def _layout(streams, tail="random", stride=STRIDE):
    """[S][stride] u8 and the lengths; the bytes between a stream's len and the stride: random (sync words and all), zeros, or
    repeated valid sealed frames"""
    S = len(streams)
    if tail == "random":
        buf = np.random.default_rng(99).integers(0, 256, (S, stride)).astype(np.uint8)
    elif tail == "zeros":
        buf = np.zeros((S, stride), np.uint8)
    else:
        f = M.frame(0, 0, 0)
        buf = np.tile(f, (S, stride // len(f) + 1))[:, :stride].copy()
    lens = np.zeros(S, np.int32)
    for i, x in enumerate(streams):
        buf[i, :len(x)] = x
        lens[i] = len(x)
    return buf, lens


def _scan(engine, buf, lens, mode, max_frames=MAX_FRAMES, prefill=0xa5):
    """-> (refs [S][max_frames] records, info [S] records, the raw refs bytes [S][max_frames][8], device tensors (streams, refs, info))"""
    import torch
    pkg = H.pkg()
    d = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    refs = torch.full((buf.shape[0], max_frames, 8), prefill, dtype=torch.uint8, device="cuda")
    info = torch.full((buf.shape[0], 24), prefill, dtype=torch.uint8, device="cuda")
    engine.frame_scan_batch(d, torch.from_numpy(lens).cuda(), mode, max_frames, refs=refs, info=info)
    engine.sync()
    raw = refs.cpu().numpy()
    return (raw.view(pkg.capi.frame_ref_dtype())[..., 0], info.cpu().numpy().view(pkg.capi.scan_info_dtype())[..., 0], raw, (d, refs, info))


def _assert_parity(got, want, prefill=0xa5):
    refs, info, raw, _ = got
    for s, (frames, winfo) in enumerate(want):
        g = {k: int(info[s][k]) for k in M.INFO_FIELDS}
        assert g == winfo, (s, g, winfo)
        n = winfo["n_frames"]
        assert [(int(r["offset"]), int(r["bytes"]), int(r["sizecod"]), int(r["reserved"])) for r in refs[s, :n]] == [f + (0,) for f in frames], s
        assert np.all(raw[s, n:] == prefill), s            # entries at or behind n_frames are left untouched
        assert g["consumed"] == g["skipped"] + sum(f[1] for f in frames)


@pytest.mark.parametrize("mode", (0, 1))
def test_model_parity(engine, mode):
    streams, want = _streams()
    buf, lens = _layout(streams)
    _assert_parity(_scan(engine, buf, lens, mode), want[mode])


@pytest.mark.parametrize("mode", (0, 1))
def test_bytes_behind_len_never_count(engine, mode):
    """the bytes between len and the stride may be read: zeros or whole valid frames there, the results are the same"""
    streams, want = _streams()
    a = _scan(engine, *_layout(streams, "zeros"), mode)
    b = _scan(engine, *_layout(streams, "frames"), mode)
    _assert_parity(a, want[mode])
    _assert_parity(b, want[mode])
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("mode", (0, 1))
def test_prefill_and_workspaces_do_not_matter(engine, mode):
    streams, want = _streams()
    buf, lens = _layout(streams)
    engine.fill_workspaces(0x00)
    a = _scan(engine, buf, lens, mode, prefill=0x00)
    engine.fill_workspaces(0xff)
    b = _scan(engine, buf, lens, mode, prefill=0xa5)
    _assert_parity(a, want[mode], 0x00)
    _assert_parity(b, want[mode], 0xa5)
    assert np.array_equal(a[1], b[1])
    for s, (frames, _) in enumerate(want[mode]):
        assert np.array_equal(a[2][s, :len(frames)], b[2][s, :len(frames)])


def test_streams_more_than_4_gib_apart(engine):
    """stream s lies at s * stream_stride, a 64-bit product: three streams 2 GiB apart, the third 2^32 bytes from the first"""
    import torch
    pkg = H.pkg()
    stride = 1 << 31
    data = [np.concatenate([M.garbage(5 + 3 * i, i), M.frame(0, 8, i & 1), M.frame(0, 4 * i, 0)]) for i in range(3)]
    d = torch.empty((3, stride), dtype=torch.uint8, device="cuda")
    for i, x in enumerate(data):
        d[i, :4096] = 0
        d[i, :len(x)] = torch.from_numpy(x).cuda()
    lens = torch.tensor([len(x) for x in data], dtype=torch.int32, device="cuda")
    for mode in (0, 1):
        refs, info = engine.frame_scan_batch(d, lens, mode, 4)
        out = engine.frame_gather_batch(d, refs, info, 2, 256)
        engine.sync()
        r = refs.cpu().numpy().view(pkg.capi.frame_ref_dtype())[..., 0]
        got = out.cpu().numpy()
        for i, x in enumerate(data):
            frames, winfo = M.scan(x, mode, 4)
            assert len(frames) == 2 and [(int(q["offset"]), int(q["bytes"])) for q in r[i, :2]] == [f[:2] for f in frames], i
            for f, (o, n, _) in enumerate(frames):
                assert np.array_equal(got[i, f, :n], x[o:o + n]) and not got[i, f, n:].any()
    del d


def test_offsets_past_2_gib_in_one_stream(engine):
    """one stream of back-to-back 3840-byte frames that ends 100 bytes past 2 GiB + 3 frames: offsets, consumed and the gather's
    addresses pass 2^31 (mode 0: one hop per frame; the expected list follows from the tiling)"""
    import torch
    pkg = H.pkg()
    f = M.frame(2, 37, 0)
    fb = len(f)
    length = (1 << 31) + 3 * fb + 100
    stride = (length + 15) & ~15
    n = length // fb
    assert length - n * fb >= 8 and n * fb > 1 << 31
    d = torch.from_numpy(f).cuda().repeat(stride // fb + 1)[:stride].view(1, stride)
    lens = torch.tensor([length - (1 << 32)], dtype=torch.int32, device="cuda")         # the same 32 bits
    refs, info = engine.frame_scan_batch(d, lens, 0, n + 4)
    out = engine.frame_gather_batch(d, refs, info, 3, fb, first_frame=n - 2)
    engine.sync()
    i = info.cpu().numpy().view(pkg.capi.scan_info_dtype())[0, 0]
    assert {k: int(i[k]) for k in M.INFO_FIELDS} == dict(n_frames=n, consumed=n * fb, skipped=0, rejected=0, flags=M.INCOMPLETE, reserved=0)
    r = refs.cpu().numpy().view(pkg.capi.frame_ref_dtype())[0, :, 0]
    assert np.array_equal(r["offset"][:n], np.arange(n, dtype=np.uint64) * fb) and np.all(r["bytes"][:n] == fb) and np.all(r["sizecod"][:n] == f[4])
    assert not refs.cpu().numpy()[0, n:].any()
    got = out.cpu().numpy()[0]
    assert np.array_equal(got[0], f) and np.array_equal(got[1], f) and not got[2].any()
    del d


def _numpy_gather(streams, lists, first, F, frame_bytes, frame_stride):
    out = np.zeros((len(streams), F, frame_stride), np.uint8)
    for s, (x, (frames, _)) in enumerate(zip(streams, lists)):
        for f in range(F):
            if first + f < len(frames):
                o, n, _ = frames[first + f]
                if n <= frame_bytes:
                    out[s, f, :n] = x[o:o + n]
    return out


@pytest.mark.parametrize("first,frame_bytes,frame_stride,shift", [(0, 1536, 1536, 0), (2, 1536, 1536, 0), (0, 3840, 3840, 0), (0, 1536, 1552, 0),
                                                                  (0, 1536, 1540, 0), (2, 3840, 3844, 4), (0, 836, 836, 12)])
def test_gather(engine, first, frame_bytes, frame_stride, shift):
    """the gathered array against a numpy gather of the model's list, byte for byte, zeros included: slots without a frame,
    frames longer than frame_bytes, frames from every byte alignment; 16-byte and (a slot stride or a stream base that is
    no multiple of 16) dword paths"""
    import torch
    streams, want = _streams()
    buf, lens = _layout(streams)
    F = 6
    _, _, _, (d, refs, info) = _scan(engine, buf, lens, 1)
    lists = want[1]
    offs = [f[0] for fr, _ in lists for f in fr[first:first + F]]
    assert {o & 3 for o in offs} == {0, 1, 2, 3} and len({o & 15 for o in offs}) > 8 and any(len(fr) < first + F for fr, _ in lists) and any(len(fr) > first + F for fr, _ in lists)
    assert any(f[1] > frame_bytes for fr, _ in lists for f in fr[first:first + F]) or frame_bytes == 3840
    if shift:                                               # the same bytes from a base that is only 4-byte aligned
        flat = torch.zeros(buf.size + 16, dtype=torch.uint8, device="cuda")
        flat[shift:shift + buf.size] = d.reshape(-1)
        d = flat[shift:shift + buf.size].view(buf.shape)
        assert d.data_ptr() % 16 == shift and d.is_contiguous()
    out = torch.full((len(streams), F, frame_stride), 0xa5, dtype=torch.uint8, device="cuda")
    engine.frame_gather_batch(d, refs, info, F, frame_bytes, first_frame=first, frame_stride=frame_stride, out=out)
    engine.sync()
    expect = _numpy_gather(streams, lists, first, F, frame_bytes, frame_stride)
    got = out.cpu().numpy()
    assert np.array_equal(got, expect), np.argwhere(got != expect)[:8]


def test_arguments(engine):
    import torch
    lib, ctx = engine.lib, ctypes.c_void_p(engine.ctx)
    d = torch.zeros((2, 64), dtype=torch.uint8, device="cuda")
    lens = torch.zeros(2, dtype=torch.int32, device="cuda")
    refs = torch.zeros((2, 4, 8), dtype=torch.uint8, device="cuda")
    info = torch.zeros((2, 24), dtype=torch.uint8, device="cuda")
    out = torch.zeros((2, 2, 128), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + o)    # noqa: E731
    ok = [ctx, p(d), 64, p(lens), 2, 0, 4, p(refs), p(info)]
    assert lib.ac3mi_frame_scan_batch(*ok) == 0
    for i, bad in ((1, None), (3, None), (7, None), (8, None), (5, 2), (5, -1), (6, 0), (4, -1), (2, 72), (1, p(d, 4)), (2, 1 << 32),
                   (7, p(refs, 2)), (8, p(info, 1))):
        args = list(ok)
        args[i] = bad
        assert lib.ac3mi_frame_scan_batch(*args) == -1, (i, bad)
        assert b"ac3mi_frame_scan_batch" in lib.ac3mi_last_error(ctx)
    args = list(ok)
    args[4] = 0
    assert lib.ac3mi_frame_scan_batch(*args) == 0
    ok = [ctx, p(d), 64, 2, p(refs), p(info), 4, 0, 2, p(out), 128, 128]
    assert lib.ac3mi_frame_gather_batch(*ok) == 0
    for i, bad in ((1, None), (4, None), (5, None), (9, None), (6, 0), (7, -1), (8, 0), (11, 7), (11, 3841), (10, 124), (10, 130), (2, 66),
                   (1, p(d, 2)), (9, p(out, 1)), (3, -1)):
        args = list(ok)
        args[i] = bad
        assert lib.ac3mi_frame_gather_batch(*args) == -1, (i, bad)
        assert b"ac3mi_frame_gather_batch" in lib.ac3mi_last_error(ctx)
    args = list(ok)
    args[3] = 0
    assert lib.ac3mi_frame_gather_batch(*args) == 0
    engine.sync()


def _real_streams(nch, bitrate, counts, seed):
    """dirty streams of real encoder frames: garbage in front of and between the frames, a cut frame in the middle of one
    stream -> (streams, per stream its whole frames [n][fb])"""
    chmap = H.CHMAP6 if nch == 6 else tuple(range(8))
    streams, frames = [], []
    for i, n in enumerate(counts):
        fr = H.orc_encode(H.gen_pcm(n, nch, seed=seed + i, kind=("music", "tones", "bursts")[i % 3]), nch, bitrate, 48000, chmap)
        parts = [M.garbage(3 + 7 * i, seed + i)]
        for k in range(n):
            parts.append(fr[k])
            if k == 1 and i == 1:
                parts.append(fr[0][:fr.shape[1] // 3])      # a frame cut short: its header runs over the next true frame
            if k % 2 == i % 2:
                parts.append(M.garbage(1 + 5 * k + i, seed + 10 * k))
        streams.append(np.concatenate(parts))
        frames.append(fr)
    return streams, frames


@pytest.mark.parametrize("nch,bitrate,acmod,lfeon", [(2, 192000, 2, 0), (6, 384000, 7, 1)])
def test_scan_gather_decode(engine, nch, bitrate, acmod, lfeon):
    """bytes -> scan (mode 1) -> gather -> ac3mi_decode_s16_batch is bit-identical to the same call on the same frames laid out
    by the host; status words equal; slots without a frame carry bit 8 and, once the overlap has faded, silence"""
    import torch
    pkg = H.pkg()
    counts = (4, 6, 3)
    F = 6
    streams, frames = _real_streams(nch, bitrate, counts, 900 + nch)
    fb = frames[0].shape[1]
    stride = (max(len(x) for x in streams) + 15) & ~15
    buf, lens = _layout(streams, "random", stride)
    refs, info, _, (d, d_refs, d_info) = _scan(engine, buf, lens, 1, max_frames=8)
    assert [int(n) for n in info["n_frames"]] == list(counts)
    gathered = engine.frame_gather_batch(d, d_refs, d_info, F, fb)
    fstride = gathered.shape[2]
    host = np.zeros((len(counts), F, fstride), np.uint8)
    for s, fr in enumerate(frames):
        host[s, :len(fr), :fb] = fr
    engine.sync()
    assert np.array_equal(gathered.cpu().numpy(), host)
    flags = pkg.syncinfo(frames[0][0])[1]
    desc = pkg.DecodeDesc(flags=flags | 32, level=1.0, bias=384.0, dynrng=1, acmod=acmod, lfeon=lfeon, frame_bytes=fb)
    n_out, _ = engine.decode_planes(desc)
    res = []
    for fr_t in (gathered, torch.from_numpy(host).cuda()):
        delay = torch.zeros((len(counts), n_out, 128), dtype=torch.float32, device="cuda")
        lfsr = torch.ones((len(counts),), dtype=torch.int16, device="cuda")
        pcm, status = engine.decode_s16_batch(desc, fr_t, delay, lfsr)
        engine.sync()
        res.append((pcm.cpu().numpy(), status.cpu().numpy(), delay.cpu().numpy(), lfsr.cpu().numpy()))
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    pcm, status = res[0][:2]
    for s, n in enumerate(counts):
        assert not (status[s, :n] & 0x13f).any() and np.abs(pcm[s, :n].astype(np.int32)).max() > 100
        assert (status[s, n:] & 0x100).all()
        assert not pcm[s, n + 1:].any()                     # (slot n fades the last frame's overlap out)


def test_against_the_stream_layer(engine):
    """one 2/0 stream, garbage between its six frames: ac3mi_stream_convert's host loop and mode 0 scan + gather +
    ac3mi_decode_s16_batch with the flags the stream layer derives give the same PCM bytes"""
    import importlib
    import torch
    pkg = H.pkg()
    S = importlib.import_module("ac-3-acm-codec_amd.stream")
    n = 6
    fr = H.orc_encode(H.gen_pcm(n, 2, seed=321, kind="music"), 2, 192000, 48000, tuple(range(8)))
    fb = fr.shape[1]
    parts = [M.garbage(23, 1)]
    for k in range(n):
        parts.append(fr[k])
        if k < n - 1:
            parts.append(M.garbage(2 + 9 * k, 50 + k))
    data = np.concatenate(parts)
    pool = S.Pool(engine, 4)
    rc, st = pool.open(S.ac3_format(2, 48000, 192, block_align=fb), S.pcm_format(2, 48000))
    assert rc == 0 and st is not None
    out, pos = bytearray(), 0
    for call in range(16):
        src = data[pos:].copy() if pos < len(data) else np.zeros(1, np.uint8)
        left = len(data) - pos
        dst = np.zeros(1 << 18, np.uint8)
        h = S.StreamHeader(src.ctypes.data, left, 0, dst.ctypes.data, dst.size, 0, S.STREAMCONVERTF_START if call == 0 else 0)
        assert st.convert(h) == 0
        out += dst[:h.dst_used].tobytes()
        pos += h.src_used
        if left == 0 and h.dst_used == 0:
            break
    st.close()
    pool.close()
    assert len(out) == n * 6 * 256 * 2 * 2                 # the stream layer produced n_frames * 6 blocks: the comparison is whole
    stride = (len(data) + 15) & ~15
    buf, lens = _layout([data], "zeros", stride)
    refs, info, _, (d, d_refs, d_info) = _scan(engine, buf, lens, 0, max_frames=8)
    assert int(info[0]["n_frames"]) == n
    frames = engine.frame_gather_batch(d, d_refs, d_info, n, fb)
    flags = pkg.syncinfo(fr[0])[1]
    desc = pkg.DecodeDesc(flags=flags | 32, level=1.0, bias=384.0, dynrng=1, acmod=2, lfeon=0, frame_bytes=fb)
    delay = torch.zeros((1, 2, 128), dtype=torch.float32, device="cuda")
    lfsr = torch.ones((1,), dtype=torch.int16, device="cuda")
    pcm, status = engine.decode_s16_batch(desc, frames, delay, lfsr)
    engine.sync()
    assert not (status.cpu().numpy() & 0x13f).any()
    assert pcm.cpu().numpy().tobytes() == bytes(out)


def test_timing_script_runs():
    """profiles/frame_scan_ab.py on a small batch: it runs and prints one parseable JSON line (no timing is asserted)"""
    r = subprocess.run([sys.executable, os.path.join(H.ROOT, "profiles", "frame_scan_ab.py"), "--frames", "256", "--passes", "2"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().split("\n")[-1])
    assert res["streams"] == 256 and res["frames_per_stream"] == 4
    for case in ("scan_mode0", "scan_mode1", "gather", "crc_check_batch", "scan_mode0_dirty", "scan_mode1_dirty"):
        assert res[case]["median_ms"] > 0 and res[case]["passes"] == 2
