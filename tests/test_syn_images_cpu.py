"""CPU: csrc/enc_syntax.h's second statement of the fixed 5.1 frame's side information - the prefix and suffix images of an
audio block, its rows' bit offsets and the header image, which enc_packf_kernel<true> ORs into the frame by lanes - against the
field lists syn_header / syn_block, the one authority.  tests/syn_images_c/main.cpp (see there for the frames) writes every
block both ways into zeroed buffers at bit positions 0, 1 and 31 modulo 32 and compares them bit for bit, the offsets of every
absolute exponent and gainrng with where the list's sink put them, and the block's length with the sink and syn_block_bits.
A program of its own, built with the host compiler under -fsanitize=address,undefined; nothing here comes from the engine."""
import os
import subprocess

import pytest

from tests import _harness as H

# one channel's strategies over six blocks, per channel: 3 * 4^5 for each full-bandwidth channel, 2^5 for the LFE;
# all-new per strategy and block-0-alone per strategy, with each of the six (csnr, fsnr) pairs
FRAMES = 5 * 3 * 4 ** 5 + 2 ** 5 + 6 * 3 * 2


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("syn_images")
    exe = str(tmp / "syn_images")
    H.build_sanitised([os.path.join(H.ROOT, "tests", "syn_images_c", "main.cpp")], exe, includes=[H.CSRC])
    return exe


def test_images_equal_the_lists(exe):
    """every frame's six blocks at the three bit positions: images, row offsets and lengths equal to what syn_block writes, the
    header image to syn_header; neither sanitiser spoke"""
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    assert r.stdout.split() == ["frames=%d" % FRAMES, "blocks=%d" % (FRAMES * 6 * 3)], r.stdout


def test_it_takes_no_arguments(exe):
    """(the frames are the program's own: nothing selects a subset)"""
    assert subprocess.run([exe, "1"], capture_output=True, text=True).returncode == 2
