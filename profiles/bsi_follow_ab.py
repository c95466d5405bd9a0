#!/usr/bin/env python3
"""The transcode with the context's metadata against the one that follows its source (ac3mi_set_encode_metadata_source 0 / 1),
and the BSI reader alone (ac3mi_bsi_read_batch), on bench.py's transcode shape - 65 536 one-frame 5.1 streams at 384 kb/s:
`python profiles/bsi_follow_ab.py [--frames N] [--passes P]`.
Times are ac3mi_timer_* (HIP events on the engine's stream) around one call, warm; every case is timed P times with the
cases interleaved (read, 0, 1, read, 0, 1, ...) and reported as median with min / max.  Mode 0 launches the kernels it always
did; mode 1 adds the BSI kernel and takes the packers' MD variants.  Prints one JSON line.
Kernel times: `rocprofv3 --kernel-trace --stats -- python profiles/bsi_follow_ab.py --passes 3` and look for bsi_kernel."""
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
args = ap.parse_args()

pkg = bench.importlib_pkg()
dev = torch.device("cuda:0")
eng = pkg.Engine(0)
S = args.frames
C = bench.Content(pkg, eng, dev, S, 0)                   # seeded PCM -> AC-3 frames, as bench.py's legs use them
frames = C.frames
info = torch.zeros((S, 1, 36), dtype=torch.uint8, device=dev)
torch.cuda.synchronize(dev)


def read():
    eng.bsi_read_batch(frames, C.fb, out=info, wait_torch=False)


def timed(fn, reset=None):
    if reset:
        reset()
    eng.timer_start()
    fn()
    return eng.timer_stop()


def stats(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "passes": len(xs)}


res = {"frames": S, "frame_bytes": C.fb, "device": torch.cuda.get_device_name(0)}
for _ in range(3):                                       # warm: every kernel of every case has run
    for mode in (0, 1):
        eng.set_encode_metadata_source(mode)
        C.reset_transcode()
        C.transcode()
    read()
eng.sync()
t = {"read": [], 0: [], 1: []}
out = {}
for _ in range(args.passes):
    t["read"].append(timed(read))
    for mode in (0, 1):
        eng.set_encode_metadata_source(mode)
        t[mode].append(timed(C.transcode, C.reset_transcode))
        eng.sync()
        out[mode] = C.frames2.clone()
eng.set_encode_metadata_source(0)
eng.sync()
assert int(info[:, 0, 0].max().item()) == 0 and int((C.status_tc & 0xfff).max().item()) == 0
# the bench's sources carry the default BSI, so following them must reproduce mode 0's bytes
assert torch.equal(out[0], out[1])
res["bsi_read_batch"] = stats(t["read"])
res["transcode"] = {"mode%d" % m: stats(t[m]) for m in (0, 1)}
res["transcode"]["mode1_minus_mode0_ms"] = res["transcode"]["mode1"]["median_ms"] - res["transcode"]["mode0"]["median_ms"]
print(json.dumps(res))
eng.close()
