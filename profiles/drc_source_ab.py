#!/usr/bin/env python3
"""The transcode that drops its source's dynrng / compr words against the one that carries them
(ac3mi_set_encode_drc_source 0 / 1), on bench.py's transcode shape - 65 536 one-frame 5.1 streams at 384 kb/s, decoded with
dynrng 0 in both modes: `python profiles/drc_source_ab.py [--frames N] [--passes P]`.
The sources carry words: bench.py's PCM encoded once under ac3mi_set_encode_dynrng_frames with a new random word in half of
the blocks and a compr word in half of the frames.  Times are ac3mi_timer_* (HIP events on the engine's stream) around one
call, warm; both modes are timed P times, interleaved (0, 1, 0, 1, ...), and reported as median with min / max.  Mode 0 is
a call with the feature off: the fixed-shape kernels.  Mode 1 adds enc_dynrng_source_kernel and takes the SRC front end and
the DW search and packer, all generic-shape; `--generic` times mode 0 with ac3mi_set_fixed_shape 0 as well, which separates
the cost of the words from the cost of leaving the fixed shape.  Prints one JSON line.
Kernel times: `rocprofv3 --kernel-trace --stats -- python profiles/drc_source_ab.py --passes 3`."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=65536)
ap.add_argument("--passes", type=int, default=15)
ap.add_argument("--generic", action="store_true")
args = ap.parse_args()

pkg = bench.importlib_pkg()
dev = torch.device("cuda:0")
eng = pkg.Engine(0)
S = args.frames
C = bench.Content(pkg, eng, dev, S, 0)                   # seeded PCM -> AC-3 frames, as bench.py's legs use them
g = torch.Generator(device=dev).manual_seed(7)
new = torch.rand((S, 1, 6, 2), generator=g, device=dev) < 0.5
word = torch.randint(0, 256, (S, 1, 6, 2), generator=g, device=dev, dtype=torch.int32)
codes = torch.zeros((S, 1, 6, 2), dtype=torch.int32, device=dev)
for b in range(6):
    codes[:, :, b] = torch.where(new[:, :, b], word[:, :, b], codes[:, :, b - 1] if b else torch.zeros_like(word[:, :, 0]))
codes = codes.to(torch.uint8).contiguous()
compr = (torch.randint(0, 512, (S, 1, 2), generator=g, device=dev, dtype=torch.int32)).to(torch.int16).contiguous()
torch.cuda.synchronize(dev)
eng.set_encode_dynrng_frames(codes, compr)
eng.memset(C.last)
C.csnr.fill_(40)
torch.cuda.synchronize(dev)
eng.encode_batch(C.enc, C.pcm, C.chmap, C.last, C.csnr, out=C.frames, wait_torch=False)
eng.sync()
eng.set_encode_dynrng_frames(None, None)
C.dec = pkg.DecodeDesc(flags=7 | 16 | 32, level=1.0, bias=384.0, dynrng=0, acmod=7, lfeon=1, frame_bytes=C.fb)


def timed(fn, reset=None):
    if reset:
        reset()
    eng.timer_start()
    fn()
    return eng.timer_stop()


def stats(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "passes": len(xs)}


def select(case):
    eng.set_encode_drc_source(1 if case == "mode1" else 0)
    eng.set_fixed_shape(0 if case == "mode0_generic" else 1)


cases = ["mode0", "mode1"] + (["mode0_generic"] if args.generic else [])
res = {"frames": S, "frame_bytes": C.fb, "device": torch.cuda.get_device_name(0)}
for _ in range(3):                                       # warm: every kernel of every case has run
    for case in cases:
        select(case)
        C.reset_transcode()
        C.transcode()
eng.sync()
t = {case: [] for case in cases}
out = {}
for _ in range(args.passes):
    for case in cases:
        select(case)
        t[case].append(timed(C.transcode, C.reset_transcode))
        eng.sync()
        out[case] = C.frames2.clone()
select("mode0")
eng.sync()
assert int((C.status_tc & 0xfff).max().item()) == 0
assert not torch.equal(out["mode0"], out["mode1"]), "mode 1 carries the words"
if args.generic:
    assert torch.equal(out["mode0"], out["mode0_generic"])
res["transcode"] = {case: stats(t[case]) for case in cases}
res["transcode"]["mode1_minus_mode0_ms"] = res["transcode"]["mode1"]["median_ms"] - res["transcode"]["mode0"]["median_ms"]
print(json.dumps(res))
eng.close()
