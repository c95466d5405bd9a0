#!/usr/bin/env python3
"""The true-peak limiter (ac3mi_limit_batch, ac3mi_limit_read_batch) on 65 536 one-frame 5.1 streams (1.2 GB of s16 PCM), beside
two yardsticks taken in the same run on the same buffer: ac3mi_truepeak_batch - the meter, whose detector the limiter repeats
before its gain computer and its stores - and ac3mi_probe_copy_rate scaled to the PCM's byte count (a bare copy moves read +
written bytes, as the limiter does).  The content is profiles/truepeak_ab.py's scaled so that part of the streams are over the
-1 dBTP ceiling (the quotient's division runs only there).
`python profiles/limit_ab.py [--streams N] [--passes P]`.
Times are ac3mi_timer_* (HIP events on the engine's stream) around one call, warm; every case is timed P times with the cases
interleaved and reported as median with min / max.  Prints one JSON line.
Kernel times: `rocprofv3 --kernel-trace --stats -- python profiles/limit_ab.py --passes 3` and look for limit_kernel /
limit_read_kernel / truepeak_kernel."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=65536)
ap.add_argument("--passes", type=int, default=15)
args = ap.parse_args()

pkg = bench.importlib_pkg()
dev = torch.device("cuda:0")
eng = pkg.Engine(0)
N, nch = args.streams, 6
g = torch.Generator(device=dev).manual_seed(99)                     # profiles/truepeak_ab.py's content, 2.5 times as loud
t = torch.arange(1536, device=dev, dtype=torch.float32)
ph = torch.rand((N, 1, 1), device=dev, generator=g) * 6.28
bed = 6000.0 * torch.sin(ph + 0.02 * t[None, :, None]) + 3000.0 * torch.sin(2 * ph + 0.31 * t[None, :, None])
bed = bed + (torch.rand((N, 1536, 1), device=dev, generator=g) - 0.5) * 4096
gains = 0.4 + 0.6 * torch.rand((N, 1, nch), device=dev, generator=g)
pcm = (2.5 * (bed * gains + (torch.rand((N, 1536, nch), device=dev, generator=g) - 0.5) * 512)).round().clamp(-32768, 32767)
x = pcm.to(torch.int16).reshape(N, 1, 1536, nch).contiguous()
del pcm, bed
x_off = torch.zeros(x.numel() + 8, dtype=torch.int16, device=dev)[1:1 + x.numel()]      # 2 bytes off: the 16-bit loads and stores
x_off.copy_(x.reshape(-1))
x_off = x_off.view(N, 1, 1536, nch)
out = torch.empty_like(x)
out_off = torch.zeros(x.numel() + 8, dtype=torch.int16, device=dev)[1:1 + x.numel()].view(N, 1, 1536, nch)
roles = pkg.loudness_roles(7 | 16)
nb = pkg.limit_state_bytes()
state = torch.zeros((N, nb), dtype=torch.uint8, device=dev)
state_off = torch.zeros_like(state)
results = torch.zeros((N, 40), dtype=torch.uint8, device=dev)
tp_state = torch.zeros((N, pkg.truepeak_state_bytes()), dtype=torch.uint8, device=dev)
ceiling = pkg.truepeak_ceiling(-1.0)
step = pkg.limit_release_step(48000, 100.0)
torch.cuda.synchronize(dev)


cases = {                                                           # (every pass limits the streams' next frame: the states carry on)
    "limit_batch": lambda: eng.limit_batch(roles, ceiling, step, x, state, out, wait_torch=False),
    "limit_batch_unaligned": lambda: eng.limit_batch(roles, ceiling, step, x_off, state_off, out_off, wait_torch=False),
    "limit_read_batch": lambda: eng.limit_read_batch(state, out=results, wait_torch=False),
    "truepeak_batch": lambda: eng.truepeak_batch(roles, x, tp_state, wait_torch=False),
}


def timed(fn):
    eng.timer_start()
    fn()
    return eng.timer_stop()


def stats(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "passes": len(xs)}


for _ in range(3):                                       # warm: every kernel of every case has run
    for fn in cases.values():
        fn()
eng.sync()
tm = {k: [] for k in cases}
for _ in range(args.passes):
    for k, fn in cases.items():
        tm[k].append(timed(fn))
eng.sync()
assert torch.equal(state, state_off) and torch.equal(out, out_off), "the two load and store paths differ"

rd = results.cpu().numpy().view(pkg.capi.limit_result_dtype())[:, 0]
copy_gbs = eng.probe_copy_rate(1 << 30)
nbytes = x.numel() * 2
res = {"streams": N, "frames_per_stream": 1, "channels": nch, "pcm_bytes": nbytes, "state_bytes": state.numel(),
       "device": torch.cuda.get_device_name(0), "copy_probe_gb_per_s_read_plus_written": copy_gbs,
       "copy_probe_ms_for_pcm_read_and_written": 2 * nbytes / (copy_gbs * 1e9) * 1e3,
       "streams_reduced": int(((rd["flags"] & 2) != 0).sum())}
for k in cases:
    res[k] = stats(tm[k])
for k in ("limit_batch", "limit_batch_unaligned", "truepeak_batch"):
    res[k]["pcm_gb_per_s"] = nbytes / (res[k]["median_ms"] * 1e-3) / 1e9
    res[k]["ns_per_frame"] = res[k]["median_ms"] * 1e6 / N
res["limit_over_truepeak"] = res["limit_batch"]["median_ms"] / res["truepeak_batch"]["median_ms"]
res["limit_over_copy_probe_time"] = res["limit_batch"]["median_ms"] / res["copy_probe_ms_for_pcm_read_and_written"]
print(json.dumps(res))
eng.close()
