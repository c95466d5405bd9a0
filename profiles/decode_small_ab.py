#!/usr/bin/env python3
"""Small decode batches in the default mode (up to 512 streams of at most four frames: decode_wg_kernel, one workgroup per
stream), for A/B runs of two builds: `python profiles/decode_small_ab.py [--calls N]` in each tree, alternating.  Per shape the
time of N back-to-back ac3mi_decode_s16_batch calls between one pair of ac3mi_timer_* events (a single call of 0.1 ms measures
the launch), five windows, median (min - max) per call in microseconds.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=400)
args = ap.parse_args()
pkg = bench.importlib_pkg()
dev = torch.device("cuda:0")
eng = pkg.Engine(0)
C = bench.Content(pkg, eng, dev, 2048, 0)
res = {"calls_per_window": args.calls, "device": torch.cuda.get_device_name(0)}
for S, F in ((64, 1), (512, 1), (128, 4), (512, 4)):
    frames = C.frames[:S * F].reshape(S, F, -1).contiguous()
    out = torch.empty((S, F, 6, 256, 6), dtype=torch.int16, device=dev)
    delay = torch.zeros((S, 6, 128), dtype=torch.float32, device=dev)
    lfsr = torch.ones((S,), dtype=torch.int16, device=dev)
    status = torch.zeros((S, F), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    for _ in range(20):
        eng.decode_s16_batch(C.dec, frames, delay, lfsr, out=out, status=status, wait_torch=False)
    eng.sync()
    us = []
    for _ in range(5):
        eng.timer_start()
        for _ in range(args.calls):
            eng.decode_s16_batch(C.dec, frames, delay, lfsr, out=out, status=status, wait_torch=False)
        us.append(eng.timer_stop() * 1e3 / args.calls)
    assert int((status & 0xfff).max().item()) == 0
    res["%dx%d" % (S, F)] = {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}
print(json.dumps(res))
eng.close()
