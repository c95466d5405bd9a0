"""CPU: ac3mi_frame_scan (host code of libac3mi.so, no GPU: the twin of frame_scan_kernel, which shares its header test)
against tests/frame_scan_model.py, in both modes - the reference's resync rule, and the same walk with CRC-confirmed sync."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import _harness as H
from tests import frame_scan_model as M

SIZES = ((0, 0), (0, 1), (0, 20), (0, 28), (0, 37), (1, 0), (1, 1), (1, 20), (1, 21), (1, 37), (2, 0), (2, 36), (2, 37))


def _scan(data, mode, max_frames=None):
    """the engine's host scan -> (frames as the model lists them, info as the model's dict)"""
    refs, info = H.pkg().frame_scan(data, mode, max_frames)
    assert refs.dtype.itemsize == 8 and np.all(refs["reserved"] == 0)
    return ([(int(r["offset"]), int(r["bytes"]), int(r["sizecod"])) for r in refs], {k: int(info[k]) for k in M.INFO_FIELDS})


def _same(data, mode, max_frames=None):
    """both scans of `data` agree, and the invariant holds -> (frames, info)"""
    want = M.scan(data, mode, max_frames if max_frames is not None else 1 << 30)
    got = _scan(data, mode, max_frames)
    assert got == want, (mode, max_frames, got[1], want[1])
    assert got[1]["consumed"] == got[1]["skipped"] + sum(f[1] for f in got[0]) and got[1]["n_frames"] == len(got[0])
    return got


def test_structs_and_exports():
    pkg = H.pkg()
    assert pkg.capi.frame_ref_dtype().itemsize == ctypes.sizeof(pkg.capi.FrameRefC) == 8
    assert pkg.capi.scan_info_dtype().itemsize == ctypes.sizeof(pkg.capi.ScanInfoC) == 24
    lib = pkg.load_library()
    for name in ("ac3mi_frame_scan", "ac3mi_frame_scan_batch", "ac3mi_frame_gather_batch"):
        assert hasattr(lib, name) and name in pkg.declared_symbols()


@pytest.mark.parametrize("fscod,code", SIZES)
def test_every_chosen_size(fscod, code):
    """garbage, then three frames of one (fscod, frmsizecod) - 128 and 3840 bytes and both sizes of a 44.1 kHz pair among them"""
    fb = M.frame_bytes(fscod, code)
    assert {(0, 0): 128, (2, 37): 3840, (1, 20): 834, (1, 21): 836}.get((fscod, code), fb) == fb
    data = np.concatenate([M.garbage(11 + code, code), M.frame(fscod, code, 0), M.frame(fscod, code, 1), M.frame(fscod, code, 0)])
    for mode in (0, 1):
        frames, info = _same(data, mode)
        assert [f[1] for f in frames] == [fb] * 3 and frames[0][0] == 11 + code and info["flags"] == 0 and info["rejected"] == 0
        assert all(f[2] == (fscod << 6 | code) for f in frames)


def test_44k_pair_alternating_in_one_stream():
    data = np.concatenate([M.frame(1, 20 + (i & 1), i) for i in range(6)] + [M.garbage(9, 3)])
    for mode in (0, 1):
        frames, info = _same(data, mode)
        assert [f[1] for f in frames] == [834, 836] * 3 and info["consumed"] == len(data) - 7


def test_dirty_stream_modes_differ():
    """mode 0 lists the planted false frame and loses the true frame it runs over; mode 1 rejects it and recovers that frame"""
    data, true_at = M.dirty_stream()
    fb = M.frame_bytes(0, 20)
    planted = true_at[1] + fb + 5
    f0, i0 = _same(data, 0)
    f1, i1 = _same(data, 1)
    assert f0 != f1
    assert planted in [f[0] for f in f0] and true_at[2] not in [f[0] for f in f0]
    assert [f[0] for f in f1] == true_at and i1["rejected"] == 2 and i0["rejected"] == 0
    assert i0["flags"] == i1["flags"] == M.INCOMPLETE and i0["consumed"] == i1["consumed"] == len(data) - 200


def test_one_broken_crc_is_enough():
    """a frame whose crc1 region alone, or crc2 region alone, is off by one bit: mode 1 rejects both, mode 0 takes them"""
    fr = [M.frame(0, 14, i) for i in range(5)]
    e1, _ = M.crc_model.regions(len(fr[0]))
    fr[1][10] ^= 0x10                           # region 1
    fr[3][e1 + 7] ^= 0x02                       # region 2
    assert M.crc_model.verdict(fr[1]) == 1 and M.crc_model.verdict(fr[3]) == 2
    data = np.concatenate(fr)
    f0, _ = _same(data, 0)
    f1, i1 = _same(data, 1)
    assert len(f0) == 5 and [f[0] for f in f1] == [0, 2 * len(fr[0]), 4 * len(fr[0])] and i1["rejected"] == 2


def test_ends():
    fr = M.frame(0, 8, 1)
    fs = len(fr)
    for mode in (0, 1):
        for n in (0, 7):
            assert _same(fr[:n], mode) == ([], dict(n_frames=0, consumed=0, skipped=0, rejected=0, flags=0, reserved=0))
        for n in (8, fs - 1):
            frames, info = _same(fr[:n], mode)
            assert frames == [] and info["consumed"] == 0 and info["flags"] == M.INCOMPLETE
        assert _same(fr, mode)[1]["consumed"] == fs
        # a valid header in the last 8 bytes
        frames, info = _same(np.concatenate([M.garbage(50, 1), fr[:8]]), mode)
        assert frames == [] and info["consumed"] == 50 and info["flags"] == M.INCOMPLETE
        # a sync word at len - 7 is not tested
        frames, info = _same(np.concatenate([M.garbage(50, 1), fr[:7]]), mode)
        assert frames == [] and info["consumed"] == 50 and info["flags"] == 0 and info["skipped"] == 50
        # only garbage
        assert _same(M.garbage(3000, 2), mode)[1] == dict(n_frames=0, consumed=2993, skipped=2993, rejected=0, flags=0, reserved=0)


@pytest.mark.parametrize("cap", (1, 3))
def test_max_frames_caps_and_resumes(cap):
    fr = [M.frame(2, 4, i) for i in range(5)]
    data = np.concatenate([M.garbage(21, 5)] + fr + [M.garbage(30, 6)])
    for mode in (0, 1):
        whole, _ = _same(data, mode)
        assert len(whole) == 5
        frames, info = _same(data, mode, cap)
        assert frames == whole[:cap] and info["flags"] == M.CAPPED and info["consumed"] == whole[cap][0]
        rest, info2 = _same(data[info["consumed"]:], mode)
        assert [(o + info["consumed"], b, c) for o, b, c in rest] == whole[cap:] and info2["flags"] == 0
    # exactly max_frames frames and nothing behind them that the walk would test: not capped
    assert _same(np.concatenate(fr[:cap]), 0, cap)[1]["flags"] == 0


def test_chunked_scan_with_the_tail_carried():
    """20 seeded random 5-way cuts: a caller that keeps [consumed, len) in front of the next chunk gets the uncut scan"""
    data, _ = M.dirty_stream(seed=1)
    rng = np.random.default_rng(2024)
    for mode in (0, 1):
        whole, winfo = _same(data, mode)
        for _ in range(20):
            cuts = [0] + sorted(rng.integers(1, len(data), 4).tolist()) + [len(data)]
            carry, base, frames = np.zeros(0, np.uint8), 0, []
            for a, b in zip(cuts[:-1], cuts[1:]):
                buf = np.concatenate([carry, data[a:b]])
                got, info = _scan(buf, mode)
                frames += [(o + base, n, c) for o, n, c in got]
                carry = buf[info["consumed"]:]
                base += info["consumed"]
            assert frames == whole and base == winfo["consumed"], (mode, cuts)


def test_argument_refusals():
    pkg = H.pkg()
    lib = pkg.load_library()
    buf = (ctypes.c_uint8 * 16)()
    refs = (pkg.capi.FrameRefC * 2)()
    info = pkg.capi.ScanInfoC()
    ok = (buf, 16, 0, 2, refs, ctypes.byref(info))
    assert lib.ac3mi_frame_scan(*ok) == 0
    for i, bad in ((0, None), (2, 2), (2, -1), (3, 0), (3, -4), (4, None), (5, None), (1, 1 << 32)):
        args = list(ok)
        args[i] = bad
        assert lib.ac3mi_frame_scan(*args) == -1, (i, bad)
    # the batched calls refuse a null context before anything else (no GPU needed to say so)
    assert lib.ac3mi_frame_scan_batch(None, None, 0, None, 0, 0, 1, None, None) == -1
    assert lib.ac3mi_frame_gather_batch(None, None, 0, 0, None, None, 1, 0, 1, None, 16, 8) == -1


def test_host_scan_under_the_sanitisers(tmp_path):
    """tests/frame_scan_c/scan_main.c with a host-only translation of csrc/scan.hip, both built with
    -fsanitize=address,undefined and run on the CPU: the model's lists, and not a word from either sanitiser"""
    exe = H.build_sanitised([os.path.join(H.ROOT, "tests", "frame_scan_c", "scan_main.c"), os.path.join(H.CSRC, "scan.hip")], str(tmp_path / "scan_main"), includes=[os.path.join(H.ROOT, "include")])
    dirty, _ = M.dirty_stream()
    fr = M.frame(1, 21, 0)
    for i, data in enumerate((dirty, dirty[1:], fr[:0], fr[:7], fr[:8], fr[:-1], fr, np.concatenate([M.garbage(50, 1), fr[:8]]))):
        path = tmp_path / ("stream%d.bin" % i)
        path.write_bytes(data.tobytes())
        for mode in (0, 1):
            for cap in (64, 2):
                r = subprocess.run([exe, str(path), str(mode), str(cap)], capture_output=True, text=True)
                assert r.returncode == 0 and r.stderr == "", (i, mode, cap, r.stdout, r.stderr)
                lines = r.stdout.split("\n")
                frames, info = M.scan(data, mode, cap)
                assert lines[0] == "info " + " ".join(str(info[k]) for k in M.INFO_FIELDS)
                assert lines[1:-1] == ["ref %d %d %d" % f for f in frames]
