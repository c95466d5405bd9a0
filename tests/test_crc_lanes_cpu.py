"""CPU: the lane rule of the packers' two CRC words, csrc/crc_lanes.h - the split of the 64 lanes between the two regions, a lane's
bytes, its constant and row, the chunk sums by dwords of the staged frame, the XOR scan - at every frame size enc_config can
return.  The checks run in tests/crc_lanes_c/main.cpp (see there), a program of its own built with the host compiler under
-fsanitize=address,undefined; it exits non-zero at the first disagreement.  Its `vec` lines are frames with the rule's words,
which the Python model (tests/crc_model.py: the definition, bit by bit) must find to seal both regions."""
import os
import subprocess

import numpy as np
import pytest

from tests import _harness as H
from tests import crc_model as M


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("crc_lanes")
    exe = str(tmp / "crc_lanes")
    H.build_sanitised([os.path.join(H.ROOT, "tests", "crc_lanes_c", "main.cpp")], exe, includes=[H.CSRC])
    r = subprocess.run([exe, "20261"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    return r.stdout.splitlines()


def test_every_frame_size_every_frame(program_output):
    """split, byte ranges, staged reads, constants; zeros, ones, 64 random frames a size, every single bit of a 128-byte frame"""
    line = program_output[-1].split()
    assert line[:2] == ["crc_lanes", "ok"]
    v = dict(tok.split("=") for tok in line[2:])
    sizes = {(k >> h) * 1000 * 1536 // ((r >> h) * 16) for h in range(3) for r in (48000, 44100, 32000) for k in M.KBPS}
    assert int(v["sizes"]) == len(sizes)
    assert int(v["frames"]) == len(sizes) * 66 + 1024
    assert int(v["c_max"]) == 60          # 32 kHz / 640 kbps: 2 400 + 1 438 bytes on 40 + 24 lanes


def test_the_words_seal_the_regions_by_the_model(program_output):
    vecs = [ln.split() for ln in program_output if ln.startswith("vec ")]
    assert sorted(int(v[1]) for v in vecs) == [64, 768, 835, 1920]
    for _, fs, crc1, crc2, hexs in vecs:
        fs, crc1, crc2 = int(fs), int(crc1), int(crc2)
        f = np.frombuffer(bytes.fromhex(hexs), np.uint8).copy()
        assert f.shape[0] == 2 * fs
        e1, e2 = M.regions(2 * fs)
        f[2], f[3], f[e2 - 2], f[e2 - 1] = crc1 >> 8, crc1 & 0xff, crc2 >> 8, crc2 & 0xff
        assert M.crc16(f[2:e1]) == 0 and M.crc16(f[e1:e2]) == 0, "fs %d" % fs
