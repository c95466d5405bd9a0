"""CPU: the header rule of csrc/sync_rule.h - which heads a52_syncinfo refuses, the frame's size, halfrate, where lfeon lies -
on every (byte 4, byte 5), against tests/stream_model.syncinfo_size and the oracle's a52_syncinfo; its masked-dword form against
its byte form; and the library's host entry points that call it (ac3mi_syncinfo, ac3mi_bsi_read, ac3mi_frame_scan) against
the same sizes.  The rule itself runs in tests/header_rule_c/main.cpp, a program of its own built with the host compiler under
-fsanitize=address,undefined; nothing here comes from the engine but what is under test."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import _harness as H
from tests.stream_model import syncinfo_size

SYNCS = (0x0b77, 0x0b76, 0x770b, 0x0000)
RATES = (48000, 44100, 32000)
BYTE5 = (0x00, 0x40, 0x58, 0x5f, 0x60, 0xff)


def _head(sync, b4, b5, b6=0, b7=0):
    return np.array([sync >> 8, sync & 0xff, 0, 0, b4, b5, b6, b7], np.uint8)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/header_rule_c/main.cpp built as tests/frame_scan_c is -> (sizes, sizes_le, fscod, halfrate, each [4][256][256]
    indexed [sync word][byte 4][byte 5]; lfeon position per acmod)"""
    tmp = tmp_path_factory.mktemp("header_rule")
    exe = str(tmp / "header_rule")
    H.build_sanitised([os.path.join(H.ROOT, "tests", "header_rule_c", "main.cpp")], exe, includes=[H.CSRC])
    r = subprocess.run([exe, "20250"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    v = np.array(r.stdout.split(), np.int64)
    assert v.size == 4 * 65536 * 4 + 8
    t = v[:-8].reshape(4, 256, 256, 4)
    return t[..., 0], t[..., 1], t[..., 2], t[..., 3], v[-8:]


def test_every_head_against_the_model_and_the_oracle(program):
    """all 65 536 (byte 4, byte 5) under the sync word: the size is the model's and the oracle's, fscod and halfrate give the
    oracle's sample rate; under three other sync words: 0"""
    size, _, fscod, halfrate, _ = program
    L = H.orc()
    for b4 in range(256):
        for b5 in range(256):
            h = _head(0x0b77, b4, b5)
            fl, sr, br = H.ci(), H.ci(), H.ci()
            want = L.orc_a52_syncinfo(H.P(h, H.u8p), ctypes.byref(fl), ctypes.byref(sr), ctypes.byref(br))
            assert size[0, b4, b5] == want == syncinfo_size(h.tolist()), (b4, b5, size[0, b4, b5], want)
            if want:
                assert fscod[0, b4, b5] == b4 >> 6 and RATES[fscod[0, b4, b5]] >> halfrate[0, b4, b5] == sr.value, (b4, b5)
    assert (size[0] != 0).sum() == 3 * 38 * 0x60
    for k, sync in enumerate(SYNCS[1:], 1):
        assert syncinfo_size(_head(sync, 0x14, 0x40).tolist()) == 0
        assert not size[k].any(), hex(sync)


def test_masked_dword_form_is_the_byte_form(program):
    """on all four sync words x 65 536 pairs, with random bytes where neither form looks"""
    size, size_le, _, _, _ = program
    differ = np.argwhere(size != size_le)
    assert differ.size == 0, "(sync word, byte 4, byte 5) %r: byte form %d, masked-dword form %d" % (
        differ[0].tolist(), size[tuple(differ[0])], size_le[tuple(differ[0])])


def test_host_entry_points(program):
    """256 values of byte 4 x six of byte 5: ac3mi_syncinfo gives the size, and flags, sample rate and bit rate as a52_syncinfo
    leaves them - on a head it refuses as well, where it has written those it reached before the refusal (parse.c:86-129; both
    sides start from zeros); ac3mi_bsi_read refuses exactly where the size is 0 and echoes fscod / frmsizecod elsewhere;
    ac3mi_frame_scan (mode 0) on the head and 3 840 zero bytes lists a frame of that size at offset 0 exactly where it is not 0"""
    pkg = H.pkg()
    L = H.orc()
    size = program[0][0]
    NOT_READ = pkg.flags.BSI_NOT_READ
    for b4 in range(256):
        for b5 in BYTE5:
            h = _head(0x0b77, b4, b5, 0xe1, 0x00)
            want = int(size[b4, b5])
            assert want == syncinfo_size(h.tolist())
            fl, sr, br = H.ci(), H.ci(), H.ci()
            assert L.orc_a52_syncinfo(H.P(h, H.u8p), ctypes.byref(fl), ctypes.byref(sr), ctypes.byref(br)) == want
            assert pkg.syncinfo(h) == (want, fl.value, sr.value, br.value), (b4, b5, pkg.syncinfo(h), fl.value, sr.value, br.value)
            info = pkg.bsi_read(h)
            if want:
                assert not (info["verdict"] & NOT_READ) and (info["fscod"], info["frmsizecod"]) == (b4 >> 6, b4 & 63), (b4, b5)
            else:
                assert info["verdict"] == NOT_READ, (b4, b5)
            refs, sinfo = pkg.frame_scan(np.concatenate([h, np.zeros(3840, np.uint8)]), 0)
            first = [(int(r["offset"]), int(r["bytes"])) for r in refs[:1] if r["offset"] == 0]
            assert first == ([(0, want)] if want else []), (b4, b5, first)
            assert sinfo["n_frames"] == len(refs)


def test_lfeon_position(program):
    """the eight acmods: the position behind acmod and the two-bit fields it sends (A/52 5.3.2), and ac3mi_syncinfo's AC3MI_LFE
    flag on heads with that one bit of bytes 6-7 set, and with it alone cleared"""
    pkg = H.pkg()
    pos = program[4]
    for acmod in range(8):
        want = 3 + 2 * ((acmod & 1 and acmod != 1) + bool(acmod & 4) + (acmod == 2))
        assert pos[acmod] == want, (acmod, pos[acmod])
        bit = 0x8000 >> want
        for rest in (0x0000, 0x1fff):
            w = (acmod << 13) | (rest & ~bit)
            for lfe in (0, 1):
                v = w | (bit if lfe else 0)
                n, flags, _, _ = pkg.syncinfo(_head(0x0b77, 0x14, 0x40, v >> 8, v & 0xff))
                assert n == 768 and bool(flags & pkg.flags.A52_LFE) == bool(lfe), (acmod, hex(v), flags)
