"""The truth for the frame-scan tests: the resync rule of stream_convert_ac3 (src/AC3ACM.cpp:1430-1628, as DecodeModel in
tests/stream_model.py follows it a byte at a time) in plain Python, with the optional CRC-confirmed sync of mode 1.

    p = 0
    while p + 8 <= len and frames listed < max_frames:
        fs = syncinfo_size(bytes p .. p + 5)
        if fs:
            if p + fs > len: stop (incomplete)
            if mode == 0 or both CRC regions of [p, p + fs) sum to 0: list (p, fs); p += fs; continue
            rejected += 1
        p += 1; skipped += 1
    consumed = p

Sizes come from stream_model.syncinfo_size, the CRC verdict from crc_model.verdict; nothing here comes from the engine.
Also the synthetic frames the tests scan: scanning never decodes, so a frame is a valid header, seeded random payload and
crc_model.seal."""
import numpy as np

from tests import crc_model
from tests.stream_model import syncinfo_size

CAPPED, INCOMPLETE = 1, 2
INFO_FIELDS = ("n_frames", "consumed", "skipped", "rejected", "flags", "reserved")

_verdicts = {}


def _crc_ok(cand):
    """crc_model.verdict(cand) == 0, remembered by the candidate's bytes (the tests scan the same frames many times)"""
    key = cand.tobytes()
    if key not in _verdicts:
        _verdicts[key] = crc_model.verdict(cand) == 0
    return _verdicts[key]


def scan(data, mode=0, max_frames=1 << 30):
    """-> (frames: list of (offset, bytes, sizecod), info: dict of INFO_FIELDS)"""
    data = np.frombuffer(bytes(bytearray(data)), np.uint8)
    n = len(data)
    # positions that hold the sync word, found at once: everything between them fails the header test on its first two bytes
    sync = set(np.nonzero((data[:-1] == 0x0b) & (data[1:] == 0x77))[0].tolist()) if n >= 2 else set()
    frames, p, skipped, rejected, flags = [], 0, 0, 0, 0
    while p + 8 <= n and len(frames) < max_frames:
        fs = syncinfo_size(data[p:p + 6].tolist()) if p in sync else 0
        if fs:
            if p + fs > n:
                flags |= INCOMPLETE
                break
            if mode == 0 or _crc_ok(data[p:p + fs]):
                frames.append((p, fs, int(data[p + 4])))
                p += fs
                continue
            rejected += 1
        p += 1
        skipped += 1
    if len(frames) == max_frames and p + 8 <= n:
        flags |= CAPPED
    info = dict(n_frames=len(frames), consumed=p, skipped=skipped, rejected=rejected, flags=flags, reserved=0)
    assert p == skipped + sum(f[1] for f in frames)
    return frames, info


def header(fscod, frmsizecod, bsid=8, acmod=2):
    """bytes 0-7 of a frame: sync word, crc1 (zero until sealed), fscod / frmsizecod, bsid / bsmod, acmod and what follows"""
    return np.array([0x0b, 0x77, 0, 0, fscod << 6 | frmsizecod, bsid << 3, acmod << 5, 0], np.uint8)


def frame_bytes(fscod, frmsizecod):
    return syncinfo_size(header(fscod, frmsizecod).tolist())


_sealed = {}


def frame(fscod, frmsizecod, seed=0):
    """a sealed synthetic frame: valid header, seeded random payload, both CRC regions summing to 0.  The payload holds no sync
    word, so that the only headers in a stream are the ones a test puts there."""
    key = (fscod, frmsizecod, seed)
    if key not in _sealed:
        n = frame_bytes(fscod, frmsizecod)
        assert n
        rng = np.random.default_rng([fscod, frmsizecod, seed])
        f = rng.integers(0, 256, n).astype(np.uint8)
        f[f == 0x0b] = 0x0c
        f[:8] = header(fscod, frmsizecod)
        f = crc_model.seal(f)
        # (the two CRC words are what they have to be: a sync word through them would be a header the test did not plant)
        assert not np.any((f[2:-1] == 0x0b) & (f[3:] == 0x77)), key
        assert crc_model.verdict(f) == 0
        _sealed[key] = f
    return _sealed[key].copy()


def garbage(n, seed):
    """n seeded random bytes without a sync word"""
    g = np.random.default_rng([7, n, seed]).integers(0, 256, n).astype(np.uint8)
    g[g == 0x0b] = 0x0d
    return g


def dirty_stream(fscod=0, frmsizecod=20, seed=0):
    """37 garbage bytes, two frames, 5 garbage bytes, a planted valid header in garbage whose size runs over the next true
    frame, two frames, a frame cut to 300 bytes, two frames, a frame cut to 200 bytes at the end
    -> (bytes, offsets of the six whole true frames in order)"""
    fr = [frame(fscod, frmsizecod, seed * 16 + i) for i in range(9)]
    fb = len(fr[0])
    assert fb > 300
    parts, true_at, pos = [], [], 0

    def put(x, is_frame=False):
        nonlocal pos
        if is_frame:
            true_at.append(pos)
        parts.append(np.asarray(x, np.uint8))
        pos += len(x)

    put(garbage(37, seed))
    put(fr[0], True)
    put(fr[1], True)
    put(garbage(5, seed + 1))
    planted = garbage(fb // 2, seed + 2)          # a header that claims fb bytes, with only fb / 2 bytes until the true frame
    planted[:8] = header(fscod, frmsizecod)
    put(planted)
    put(fr[2], True)
    put(fr[3], True)
    put(fr[4][:300])
    put(fr[5], True)
    put(fr[6], True)
    put(fr[7][:200])
    return np.concatenate(parts), true_at
