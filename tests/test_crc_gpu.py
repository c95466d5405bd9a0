"""GPU: ac3mi_crc_check_batch and ac3mi_set_decode_crc against tests/crc_model.py (CRC-16 from A/52's definition).
Mode 1 (report) leaves every output of mode 0 alone and adds status bits 10 / 11; mode 2 (conceal) equals mode 0 on the same
batch with bytes 0-1 of every failing frame zeroed.  Damaged frames are inputs the decoder is specified to survive."""
import ctypes
import os

import numpy as np
import pytest

from tests import _harness as H
from tests import crc_model as M

pytestmark = pytest.mark.gpu

CRC_BITS = 0xc00
DECODE_MODES = (0, 1, 3, 4, 5, 6)


def _pad(frames, stride=None):
    """[n][fb] -> [n][stride] zero padded (stride: fb rounded up to 4)"""
    n, fb = frames.shape
    stride = stride or (fb + 3) & ~3
    out = np.zeros((n, stride), np.uint8)
    out[:, :fb] = frames
    return out


def _check(engine, frames, frame_bytes):
    import torch
    v = engine.crc_check_batch(torch.from_numpy(np.ascontiguousarray(frames)).cuda(), frame_bytes)
    engine.sync()
    return v.cpu().numpy()


def _encoder_frames(nch, bitrate, freq, nframes, seed, kind=None):
    chmap = H.CHMAP6 if nch == 6 else tuple(range(8))
    kind = kind or ("music", "tones", "noise", "quiet", "bursts")[seed % 5]
    return H.orc_encode(H.gen_pcm(nframes, nch, seed=400 + seed, kind=kind), nch, bitrate, freq, chmap)


def _damage_tail(frames, rows, rng, lo=0.45, hi=0.97, nbytes=3):
    """flips a few bytes in the part of the frame that holds the mantissas of the later blocks"""
    fb = frames.shape[-1]
    for r in rows:
        for _ in range(nbytes):
            frames[r, int(rng.integers(int(lo * fb), int(hi * fb)))] ^= np.uint8(rng.integers(1, 256))


@pytest.mark.parametrize("nch,bitrate,freq", [(1, 96000, 48000), (2, 192000, 48000), (3, 256000, 48000), (4, 320000, 48000),
                                              (5, 448000, 48000), (6, 384000, 48000), (6, 640000, 48000), (2, 160000, 44100),
                                              (6, 448000, 44100), (2, 128000, 32000), (6, 384000, 32000), (1, 48000, 24000)])
def test_check_batch_on_encoder_frames(engine, nch, bitrate, freq):
    """intact frames of every channel count and sample rate, one flipped bit at each region's first and last bit and in the bytes
    around 2 fs58, and seeded multi-burst damage: the verdict bytes are the model's (detection is not assumed)."""
    frames = _encoder_frames(nch, bitrate, freq, 4, nch + freq // 1000)
    fb = frames.shape[1]
    e1, e2 = M.regions(fb)
    rows = [frames[i % 4].copy() for i in range(4)]
    for bit in (16, 31, 48, 8 * e1 - 1, 8 * e1, 8 * e2 - 1) + tuple(8 * b + k for b in range(e1 - 3, e1 + 3) for k in (0, 7)):
        f = frames[bit % 4].copy()
        f[bit >> 3] ^= np.uint8(0x80 >> (bit & 7))
        rows.append(f)
    rng = np.random.default_rng(fb)
    for i in range(40):
        f = frames[i % 4].copy()
        for _ in range(int(rng.integers(1, 5))):
            p = int(rng.integers(2, fb - 4))
            f[p:p + 3] ^= rng.integers(0, 256, 3).astype(np.uint8)
        rows.append(f)
    batch = _pad(np.stack(rows))
    want = M.verdicts(batch, fb)
    assert want[:4].tolist() == [0, 0, 0, 0] and want[4:10].tolist() == [1, 1, 1, 1, 2, 2]
    got = _check(engine, batch, fb)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    # the same frames on a stride that is not a multiple of 16 (dword loads) and on one that is
    for stride in (((fb + 3) & ~3) + 4, ((fb + 15) & ~15) + 16):
        assert np.array_equal(_check(engine, _pad(np.stack(rows), stride), fb), want), stride


def test_check_batch_on_sealed_packer_streams_and_non_frames(engine):
    """sealed packer streams incl. half-rate bsids, a 44.1 kHz batch with both frame sizes interleaved, non-frames (bit 7)"""
    from tests import packer
    for acmod, lfe, kw in ((7, 1, dict(bsid=9, frmsizecod=24)), (2, 0, dict(bsid=10, frmsizecod=16)), (0, 0, {}), (5, 1, dict(fscod=2, frmsizecod=26))):
        raw = packer.make_stream(8100 + acmod, 4, acmod, lfe, **kw)
        both = np.concatenate([raw, np.stack([M.seal(f) for f in raw])])
        got = _check(engine, _pad(both), raw.shape[1])
        assert np.array_equal(got, M.verdicts(both)) and got[4:].tolist() == [0] * 4 and np.count_nonzero(got[:4]) >= 3
    rng = np.random.default_rng(441)
    a = [M.seal(packer.make_frame(rng, 2, 0, fscod=1, frmsizecod=20)) for _ in range(3)]
    b = [M.seal(packer.make_frame(rng, 2, 0, fscod=1, frmsizecod=21)) for _ in range(3)]
    batch = np.zeros((8, 836), np.uint8)
    for i, f in enumerate((a[0], b[0], a[1], b[1], a[2], b[2])):
        batch[i, :f.shape[0]] = f
    batch[2, 833] ^= 4                  # last byte of the short frame
    batch[3, 835] ^= 4                  # last byte of the long one
    batch[4, 2 * ((417 >> 1) + (417 >> 3)) - 1] ^= 1        # last byte of region 1 of the short frame
    batch[6] = rng.integers(0, 256, 836)                     # noise
    batch[7, :6] = (0x0b, 0x77, 0, 0, 0x40 | 39, 0x40)       # reserved frmsizecod
    want = M.verdicts(batch, 836)
    assert want.tolist() == [0, 0, 2, 2, 1, 0, 0x80, 0x80]
    assert np.array_equal(_check(engine, batch, 836), want)
    short = M.verdicts(batch, 834)
    assert short.tolist() == [0, 0x80, 2, 0x80, 1, 0x80, 0x80, 0x80]
    assert np.array_equal(_check(engine, batch, 834), short)
    hdr = np.repeat(batch[:1], 5, axis=0)
    hdr[1, 0] = 0x0a
    hdr[2, 5] = 0x60                    # bsid 12
    hdr[3, 4] |= 0xc0                   # fscod 3
    hdr[4, 1] = 0
    assert _check(engine, hdr, 836).tolist() == M.verdicts(hdr, 836).tolist() == [0, 0x80, 0x80, 0x80, 0x80]


def test_check_batch_65536_frames(engine):
    """65 536 frames in one call, a seeded 1 % of them damaged"""
    base = _encoder_frames(6, 384000, 48000, 16, 3)
    rng = np.random.default_rng(65536)
    batch = base[rng.integers(0, 16, 65536)]
    hit = rng.choice(65536, 655, replace=False)
    for r in hit:
        batch[r, int(rng.integers(2, 1536))] ^= np.uint8(rng.integers(1, 256))
    want = M.verdicts(batch)
    got = _check(engine, batch, 1536)
    assert np.array_equal(got, want)
    assert set(np.nonzero(got)[0].tolist()) == set(hit.tolist())


def _restore(engine):
    engine.set_decode_crc(0)
    engine.set_decode_mode(int(os.environ.get("AC3MI_DECODE_MODE", "0")))
    engine.set_tile_frames(131072)
    engine.set_mix_state(None, None)
    engine._check(engine.lib.ac3mi_set_state_slots(ctypes.c_void_p(engine.ctx), None))


def _decode(engine, batch, F, fb, acmod=7, lfe=1, flags=7 | 16, s16=False, slots=False, mix=False, taps=False):
    """batch [S*F][stride] -> dict of host arrays; non-zero overlap state and per-stream dither states coming in"""
    import torch
    pkg = H.pkg()
    S = batch.shape[0] // F
    d_frames = torch.from_numpy(batch.reshape(S, F, batch.shape[1])).cuda()
    desc = pkg.DecodeDesc(flags=flags, level=1.0, bias=384.0 if s16 else 0.0, dynrng=1, acmod=acmod, lfeon=lfe, frame_bytes=fb)
    n_out, _ = engine.decode_planes(desc)
    g = torch.Generator().manual_seed(11)
    delay = ((torch.rand((S, n_out, 128), generator=g) - 0.5) * 0.25).cuda()
    lfsr = (torch.arange(S, dtype=torch.int32) * 7 + 1).to(torch.int16).cuda()
    res = {}
    if slots:
        perm = torch.randperm(S, generator=g).to(torch.int32).cuda()
        engine._check(engine.lib.ac3mi_set_state_slots(ctypes.c_void_p(engine.ctx), ctypes.c_void_p(perm.data_ptr())))
    if mix:
        pending = torch.zeros((S, n_out, 128), dtype=torch.float32, device="cuda")
        mflags = torch.zeros((S, 6), dtype=torch.int32, device="cuda")
        engine.set_mix_state(pending, mflags)
    try:
        if s16:
            pcm, status = engine.decode_s16_batch(desc, d_frames, delay, lfsr)
        elif taps:
            pcm, status, t = engine.decode_batch(desc, d_frames, delay, lfsr, taps=True)
        else:
            pcm, status = engine.decode_batch(desc, d_frames, delay, lfsr)
        engine.sync()
    finally:
        if slots:
            engine._check(engine.lib.ac3mi_set_state_slots(ctypes.c_void_p(engine.ctx), None))
        if mix:
            engine.set_mix_state(None, None)
    res.update(pcm=pcm.cpu().numpy(), status=status.cpu().numpy().astype(np.uint32).reshape(-1), delay=delay.cpu().numpy(), lfsr=lfsr.cpu().numpy())
    if taps:
        res.update(coef=t["coef"].cpu().numpy(), blksw=t["blksw"].cpu().numpy())
    if mix:
        res.update(pending=pending.cpu().numpy(), mflags=mflags.cpu().numpy())
    return res


def _same(a, b, what, skip_status_bits=0):
    for k in a:
        x, y = a[k], b[k]
        if k == "status":
            x, y = x & ~np.uint32(skip_status_bits), y & ~np.uint32(skip_status_bits)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, k, np.argwhere(x != y)[:4].tolist())


def _damaged_batch(F, seed=5):
    """5.1 encoder streams + a packer stream's frames, some damaged: mantissa bytes of the later blocks (most), the first 5/8
    (some), a refused header, a frame of another acmod.  -> (batch [S*F][1536], fb, model verdicts, rows damaged in the tail)"""
    from tests import packer
    S = 12
    rng = np.random.default_rng(seed)
    streams = [_encoder_frames(6, 384000, 48000, F, 40 + s, ("tones", "music", "noise", "bursts")[s % 4]) for s in range(S - 2)]
    streams += [np.stack([M.seal(f) for f in packer.make_stream(9000 + s, F, 7, 1, frmsizecod=28)]) for s in range(2)]
    batch = np.concatenate(streams)
    n = batch.shape[0]
    tail = [r for r in range(n) if r % 3 == 1][:max(4, n // 3)]
    _damage_tail(batch, tail, rng)
    front = [r for r in range(n) if r % 7 == 3 and r not in tail][:3]
    for r in front:
        batch[r, int(rng.integers(8, 900))] ^= np.uint8(0x10)
    if n > 8:
        batch[8, 0] = 0                                      # no sync word: refused, not summed
    other = _encoder_frames(2, 384000, 48000, 1, 1)[0]       # a 2/0 frame of the same size in a 3/2+LFE batch
    batch[n - 1] = other
    batch[n - 1, 1000] ^= 1                                  # ... and damaged: still neither bit (not summed in a decode call)
    v = M.verdicts(batch)
    return batch, 1536, v, tail


@pytest.mark.parametrize("F", [1, 4])
@pytest.mark.parametrize("s16", [False, True])
@pytest.mark.parametrize("mode", DECODE_MODES)
def test_report_and_conceal_under_every_front_end(engine, mode, s16, F):
    """mode 1: outputs and state of mode 0, status differs in bits 10 / 11 only and those are the model's.
    mode 2: mode 0 on the batch with the failing frames' sync words zeroed, bit for bit, status apart from bits 10 / 11."""
    batch, fb, v, tail = _damaged_batch(F)
    n = batch.shape[0]
    want_bits = ((v & 3).astype(np.uint32) << 10)
    want_bits[n - 1] = 0                                     # the foreign acmod: refused by the header test, not summed
    if n > 8:
        assert v[8] == 0x80
    assert v[n - 1] == 2 and np.count_nonzero(want_bits) >= len(tail)
    zeroed = batch.copy()
    zeroed[want_bits != 0, :2] = 0
    try:
        engine.set_decode_mode(mode)
        engine.set_decode_crc(0)
        plain = _decode(engine, batch, F, fb, s16=s16)
        ref2 = _decode(engine, zeroed, F, fb, s16=s16)
        assert not (plain["status"] & CRC_BITS).any()
        engine.set_decode_crc(1)
        rep = _decode(engine, batch, F, fb, s16=s16)
        _same(rep, plain, "report", CRC_BITS)
        assert np.array_equal(rep["status"] & CRC_BITS, want_bits), np.nonzero((rep["status"] & CRC_BITS) != want_bits)[0][:8]
        assert (rep["status"][n - 1] & 0x100) and (n <= 8 or rep["status"][8] & 0x100)
        engine.set_decode_crc(2)
        con = _decode(engine, batch, F, fb, s16=s16)
        _same(con, ref2, "conceal", CRC_BITS)
        assert np.array_equal(con["status"] & CRC_BITS, want_bits)
        assert ((con["status"][want_bits != 0] & 0x13f) == 0x13f).all()
        # what the feature exists for: damage that mode 0 decodes with a clean status to something else than silence
        clean = [r for r in tail if (plain["status"][r] & 0x3ff) == 0]
        pcm = plain["pcm"].reshape(n, -1)
        silent = con["pcm"].reshape(n, -1)
        loud = [r for r in clean if not np.array_equal(pcm[r], silent[r])]
        print("decode mode %d, %d frames per stream: %d of %d tail-damaged frames decode with a clean status in mode 0, %d of them not to "
              "silence" % (mode, F, len(clean), len(tail), len(loud)))
        assert loud
    finally:
        _restore(engine)


@pytest.mark.parametrize("mode", [0, 4, 5])
@pytest.mark.parametrize("variant", ["slots", "mix", "tiled", "taps"])
def test_conceal_with_slots_mix_state_tiles_and_taps(engine, variant, mode):
    """the same equivalence with state slots, the liba52-exact mix state (5.1 -> STEREO), a tiled call and stage taps - under the
    default front end (12 streams of 3 frames: one workgroup per stream), the split one and the frame-parallel one"""
    F = 3
    batch, fb, v, tail = _damaged_batch(F, seed=9)
    n = batch.shape[0]
    want_bits = ((v & 3).astype(np.uint32) << 10)
    want_bits[n - 1] = 0
    zeroed = batch.copy()
    zeroed[want_bits != 0, :2] = 0
    kw = dict(slots=dict(slots=True, s16=True), mix=dict(mix=True, flags=2), tiled=dict(s16=True), taps=dict(taps=True))[variant]
    try:
        engine.set_decode_mode(mode)
        if variant == "tiled":
            engine.set_tile_frames(2 * F)
        for crc, data in ((1, batch), (2, batch)):
            engine.set_decode_crc(0)
            want = _decode(engine, batch if crc == 1 else zeroed, F, fb, **kw)
            engine.set_decode_crc(crc)
            got = _decode(engine, data, F, fb, **kw)
            _same(got, want, (variant, crc), CRC_BITS)
            assert np.array_equal(got["status"] & CRC_BITS, want_bits), (variant, crc)
    finally:
        _restore(engine)


def _transcode(engine, batch, F, fb):
    import torch
    pkg = H.pkg()
    S = batch.shape[0] // F
    dec = pkg.DecodeDesc(flags=7 | 16, level=1.0, bias=384.0, dynrng=1, acmod=7, lfeon=1, frame_bytes=fb)
    enc = pkg.EncodeDesc(48000, 448000, 6)
    delay = torch.zeros((S, 6, 128), dtype=torch.float32, device="cuda")
    lfsr = torch.ones((S,), dtype=torch.int16, device="cuda")
    last = torch.zeros((S, 6, 256), dtype=torch.int16, device="cuda")
    csnr = torch.full((S,), 40, dtype=torch.int32, device="cuda")
    out, status = engine.transcode_batch(dec, enc, torch.from_numpy(batch.reshape(S, F, -1)).cuda(), delay, lfsr, H.CHMAP6, last, csnr)
    engine.sync()
    res = dict(frames=out.cpu().numpy().reshape(S * F, -1), status=status.cpu().numpy().astype(np.uint32).reshape(-1),
               delay=delay.cpu().numpy(), lfsr=lfsr.cpu().numpy(), last=last.cpu().numpy(), csnr=csnr.cpu().numpy())
    verdict = engine.crc_check_batch(out.reshape(S * F, -1), enc.frame_bytes())
    engine.sync()
    return res, verdict.cpu().numpy()


@pytest.mark.parametrize("F", [1, 3])
def test_transcode_conceals_instead_of_laundering(engine, F):
    """mode 0 re-encodes a mantissa-damaged frame into a frame with valid CRCs and a clean status (pinned: today's behaviour);
    mode 2 codes silence for it, byte-identical to the transcode of the sync-zeroed batch, and flags exactly the damaged inputs."""
    batch, fb, v, tail = _damaged_batch(F, seed=21)
    n = batch.shape[0]
    want_bits = ((v & 3).astype(np.uint32) << 10)
    want_bits[n - 1] = 0
    zeroed = batch.copy()
    zeroed[want_bits != 0, :2] = 0
    try:
        engine.set_decode_crc(0)
        plain, pv = _transcode(engine, batch, F, fb)
        ref2, _ = _transcode(engine, zeroed, F, fb)
        assert not pv.any(), "the encoder writes valid CRCs whatever it is fed"
        laundered = [r for r in tail if (plain["status"][r] & 0xfff) == 0]
        print("transcode, %d frames per stream: %d of %d tail-damaged frames leave mode 0 with a clean status" % (F, len(laundered), len(tail)))
        assert laundered
        engine.set_decode_crc(2)
        con, cv = _transcode(engine, batch, F, fb)
        _same(con, ref2, "transcode conceal", CRC_BITS)
        assert not cv.any()
        assert np.array_equal(con["status"] & CRC_BITS, want_bits)
        assert np.array_equal(np.nonzero(con["status"] & CRC_BITS)[0], np.nonzero(want_bits)[0])
        engine.set_decode_crc(1)
        rep, _ = _transcode(engine, batch, F, fb)
        _same(rep, plain, "transcode report", CRC_BITS)
        assert np.array_equal(rep["status"] & CRC_BITS, want_bits)
    finally:
        _restore(engine)


@pytest.mark.parametrize("crc", [1, 2])
def test_intact_input_sets_no_bit(engine, crc):
    """intact frames under modes 1 and 2: no bit anywhere, nothing concealed - 5.1 and the reference encoder's stereo frames,
    among them frames whose bit budget overshoots so that crc2 lands on the last mantissa bytes (block 5 ends behind the 18 bits
    of auxdatae, crcrsv and crc2, found with tests/ac3_syntax.py): they still carry valid CRCs"""
    from tests import ac3_syntax as A
    cases = [(6, 384000, 48000, 7, 1, "noise"), (2, 192000, 48000, 2, 0, "noise"), (2, 128000, 32000, 2, 0, "tones"),
             (2, 64000, 48000, 2, 0, "noise"), (2, 160000, 44100, 2, 0, "music"), (2, 128000, 48000, 2, 0, "tones")]
    overshoot = 0
    try:
        for nch, bitrate, freq, acmod, lfe, kind in cases:
            F = 4
            frames = np.concatenate([_encoder_frames(nch, bitrate, freq, F, 60 + s, kind) for s in range(6)])
            fb = frames.shape[1]
            assert not M.verdicts(frames).any()
            if nch == 2:
                over = [A.parse_frame(f).blocks[5].end > 8 * fb - A.TAIL_BITS for f in frames]
                overshoot += sum(over)
            batch = _pad(frames)
            for mode in (0, 3, 4):
                engine.set_decode_mode(mode)
                engine.set_decode_crc(0)
                want = _decode(engine, batch, F, fb, acmod=acmod, lfe=lfe, flags=acmod | (16 if lfe else 0))
                engine.set_decode_crc(crc)
                got = _decode(engine, batch, F, fb, acmod=acmod, lfe=lfe, flags=acmod | (16 if lfe else 0))
                _same(got, want, (nch, bitrate, freq, mode))
                assert (got["status"] & 0xfff).max() == 0
        print("stereo frames whose bit budget overshoots: %d" % overshoot)
        assert overshoot >= 3
    finally:
        _restore(engine)


def test_setter_rejects_other_modes(engine):
    lib, ctx = engine.lib, ctypes.c_void_p(engine.ctx)
    batch, fb, v, tail = _damaged_batch(1)
    try:
        assert lib.ac3mi_set_decode_crc(ctx, 2) == 0
        for bad in (-1, 3, 7):
            assert lib.ac3mi_set_decode_crc(ctx, bad) == -1       # AC3MI_ERR_ARG
        assert lib.ac3mi_set_decode_crc(None, 1) == -1
        got = _decode(engine, batch, 1, fb)                        # still mode 2: failing frames are refused
        fails = (v & 3) != 0
        fails[-1] = False
        assert ((got["status"][fails] & 0x13f) == 0x13f).all() and (got["status"][fails] & CRC_BITS).all()
    finally:
        _restore(engine)


def test_byte_stream_layer_never_checks(engine):
    """The byte-stream layer is the ACM codec's: a pool built on a context with ac3mi_set_decode_crc 1 or 2 converts a
    mantissa-damaged stream to the bytes, counts and result codes of mode 0 - the damaged frame is neither flagged nor
    silenced - through ac3mi_stream_convert and ac3mi_stream_convert_many; the setting itself survives the calls."""
    import importlib
    S = importlib.import_module(H.pkg().__name__ + ".stream")
    frames = _encoder_frames(6, 384000, 48000, 4, 77, "tones")
    intact = frames.copy()
    rng = np.random.default_rng(8)
    _damage_tail(frames, [1, 2], rng, lo=0.7, hi=0.95)
    assert M.verdicts(frames).tolist() == [0, 2, 2, 0]
    fmt = (S.ac3_format(6, 48000, 384, block_align=1536), S.pcm_format(6, 48000))
    nbytes = 4 * 6 * 256 * 12

    def convert(pool, data, many):
        rc, st = pool.open(*fmt)
        assert rc == 0
        src = np.frombuffer(data.tobytes(), np.uint8).copy()
        dst = np.zeros(nbytes, np.uint8)
        h = S.StreamHeader(src.ctypes.data, src.size, 0, dst.ctypes.data, dst.size, 0, S.STREAMCONVERTF_START)
        rc = pool.convert_many([st], [h]) if many else st.convert(h)
        st.close()
        return rc, h.src_used, h.dst_used, dst

    pool = S.Pool(engine, 4)
    try:
        res = {}
        for crc in (0, 1, 2):
            engine.set_decode_crc(crc)
            res[crc] = [convert(pool, frames, many) for many in (False, True)]
        clean = convert(pool, intact, False)
        # the setting is still there for the batched calls
        batch, fb, v, tail = _damaged_batch(1)
        got = _decode(engine, batch, 1, fb)
        assert (got["status"][tail[0]] & 0x13f) == 0x13f and (got["status"][tail[0]] & CRC_BITS)
    finally:
        _restore(engine)
        pool.close()
    for crc in (1, 2):
        for a, b in zip(res[0], res[crc]):
            assert a[:3] == b[:3] == (0, frames.size, nbytes), (crc, a[:3], b[:3])
            assert np.array_equal(a[3], b[3]), crc
    assert np.array_equal(res[0][0][3], res[0][1][3])
    # the damaged frames came through as (different) audio, not as silence
    per_frame = res[2][0][3].reshape(4, -1)
    assert per_frame[1].any() and per_frame[2].any()
    assert not np.array_equal(per_frame[1], clean[3].reshape(4, -1)[1])
