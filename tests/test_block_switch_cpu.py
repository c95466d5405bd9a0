"""CPU: the block-switch setter is part of the ABI, and the numpy model of its transient detector (tests/block_switch_model.py,
the definition in include/ac3mi.h) decides hand-built cases as A/52's thresholds say."""
import os
import re
import subprocess

import numpy as np

from tests import _harness as H
from tests import block_switch_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_setter_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ac3mi.h")).read()
    assert re.search(r"int\s+ac3mi_set_encode_block_switch\s*\(\s*ac3mi_ctx\s*\*\s*ctx\s*,\s*int\s+mode\s*\)\s*;", hdr)
    pkg = H.pkg()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "ac3mi_set_encode_block_switch" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "ac3mi_set_encode_block_switch" in pkg.declared_symbols()


def _z(h, x):
    return np.concatenate([np.asarray(h, np.int64), np.asarray(x, np.int64)])


def test_detector_silence():
    assert M.detect(np.zeros(512, np.int64)) == 0
    # loud but below the silence threshold after the high-pass: a slow full-scale sine
    t = np.arange(512)
    assert M.detect(np.round(30000 * np.sin(2 * np.pi * t / 2048.0))) == 0


def test_detector_step_in_block():
    x = np.zeros(256, np.int64)
    x[200:] = 5000                              # y = 5000 at the step, -5000 one later: far above 10 x the quiet half
    assert M.detect(_z(np.zeros(256), x)) == 1
    x[200:] = 100                               # the same step under the silence threshold
    assert M.detect(_z(np.zeros(256), x)) == 0


def test_detector_impulse_after_silence():
    x = np.zeros(256, np.int64)
    x[37] = 20000
    assert M.detect(_z(np.zeros(256), x)) == 1


def test_detector_equal_impulses_in_consecutive_blocks():
    h = np.zeros(256, np.int64)
    x = np.zeros(256, np.int64)
    h[230] = 20000
    x[230] = 20000
    assert M.detect(_z(np.zeros(256), h)) == 1  # the first one
    # the second one is as loud as the first, but the finest level compares 64-sample segments: it follows the quiet
    # [384, 448) and is a transient again
    assert M.detect(_z(h, x)) == 1
    # a steady train, one impulse per 64 samples, is not: every segment holds one
    tr = np.zeros(512, np.int64)
    tr[30::64] = 20000
    assert M.detect(tr) == 0


def test_detector_level_jump_at_64_sample_boundary():
    t = np.arange(512)
    s = 1000 * np.sin(2 * np.pi * 5000.0 / 48000.0 * t)
    for q in range(4):                          # the jump at the start of each quarter of the new half
        z = np.where(t >= 256 + 64 * q, 16 * s, s)
        assert M.detect(np.round(z)) == 1, q
    assert M.detect(np.round(16 * s)) == 0      # the same level throughout: no transient
    assert M.detect(np.round(s)) == 0


def test_decisions_follow_history():
    """Block 0 of a frame looks back at `last` (or block 5 of the frame before): a signal that carries on from its history
    switches nowhere, the same signal after zeros switches its first block."""
    t = np.arange(2 * 1536 + 256)
    sig = np.round(8000 * np.sin(2 * np.pi * 3000.0 / 48000.0 * t)).astype(np.int16)
    pcm = sig[256:].reshape(-1, 1)
    assert M.decisions(pcm, (0,), 1, last=sig[None, :256]).sum() == 0
    d = M.decisions(pcm, (0,), 1)
    assert d[0, 0, 0] == 1 and d.sum() == 1
