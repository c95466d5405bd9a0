#!/usr/bin/env python3
"""The true-peak meter (ac3mi_truepeak_batch, ac3mi_truepeak_read_batch) on 65 536 one-frame 5.1 streams (1.2 GB of s16 PCM),
beside two yardsticks taken in the same run: ac3mi_loudness_batch on the same PCM - the other kernel that reads it once, one
wavefront per stream, with a float64 cascade where this one has 48 integer multiply-adds per sample and slot - and
ac3mi_probe_copy_rate scaled to the PCM's byte count (a bare copy moves read + written bytes; the meter only reads).
`python profiles/truepeak_ab.py [--streams N] [--passes P]`.
Times are ac3mi_timer_* (HIP events on the engine's stream) around one call, warm; every case is timed P times with the cases
interleaved and reported as median with min / max.  Prints one JSON line.
Kernel times: `rocprofv3 --kernel-trace --stats -- python profiles/truepeak_ab.py --passes 3` and look for truepeak_kernel /
truepeak_read_kernel / loudness_kernel."""
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
g = torch.Generator(device=dev).manual_seed(99)                     # profiles/loudness_ab.py's content
t = torch.arange(1536, device=dev, dtype=torch.float32)
ph = torch.rand((N, 1, 1), device=dev, generator=g) * 6.28
bed = 6000.0 * torch.sin(ph + 0.02 * t[None, :, None]) + 3000.0 * torch.sin(2 * ph + 0.31 * t[None, :, None])
bed = bed + (torch.rand((N, 1536, 1), device=dev, generator=g) - 0.5) * 4096
gains = 0.4 + 0.6 * torch.rand((N, 1, nch), device=dev, generator=g)
pcm = (bed * gains + (torch.rand((N, 1536, nch), device=dev, generator=g) - 0.5) * 512).round().clamp(-32768, 32767)
x = pcm.to(torch.int16).reshape(N, 1, 1536, nch).contiguous()
del pcm, bed
x_off = torch.zeros(x.numel() + 8, dtype=torch.int16, device=dev)[1:1 + x.numel()]      # 2 bytes off: the 16-bit loads
x_off.copy_(x.reshape(-1))
x_off = x_off.view(N, 1, 1536, nch)
roles = pkg.loudness_roles(7 | 16)
state = torch.zeros((N, pkg.truepeak_state_bytes()), dtype=torch.uint8, device=dev)
state_off = torch.zeros_like(state)
results = torch.zeros((N, 96), dtype=torch.uint8, device=dev)
loud_state = torch.zeros((N, pkg.loudness_state_bytes()), dtype=torch.uint8, device=dev)
ceiling = pkg.truepeak_ceiling(-1.0)
torch.cuda.synchronize(dev)

cases = {
    "truepeak_batch": lambda: eng.truepeak_batch(roles, x, state, wait_torch=False),
    "truepeak_batch_unaligned": lambda: eng.truepeak_batch(roles, x_off, state_off, wait_torch=False),
    "truepeak_read_batch": lambda: eng.truepeak_read_batch(state, ceiling, out=results, wait_torch=False),
    "loudness_batch": lambda: eng.loudness_batch(48000, roles, x, loud_state, wait_torch=False),
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
assert torch.equal(state, state_off), "the two load paths differ"

copy_gbs = eng.probe_copy_rate(1 << 30)
nbytes = x.numel() * 2
res = {"streams": N, "frames_per_stream": 1, "channels": nch, "pcm_bytes": nbytes, "state_bytes": state.numel(),
       "device": torch.cuda.get_device_name(0), "copy_probe_gb_per_s_read_plus_written": copy_gbs,
       "copy_probe_ms_for_pcm_bytes": nbytes / (copy_gbs * 1e9) * 1e3}
for k in cases:
    res[k] = stats(tm[k])
for k in ("truepeak_batch", "truepeak_batch_unaligned", "loudness_batch"):
    res[k]["pcm_gb_per_s"] = nbytes / (res[k]["median_ms"] * 1e-3) / 1e9
    res[k]["pcm_rate_over_copy_probe"] = res[k]["pcm_gb_per_s"] / copy_gbs
    res[k]["ns_per_frame"] = res[k]["median_ms"] * 1e6 / N
res["truepeak_read_batch"]["state_gb_per_s"] = state.numel() / (res["truepeak_read_batch"]["median_ms"] * 1e-3) / 1e9
res["truepeak_over_loudness"] = res["truepeak_batch"]["median_ms"] / res["loudness_batch"]["median_ms"]
res["truepeak_over_copy_probe_time"] = res["truepeak_batch"]["median_ms"] / res["copy_probe_ms_for_pcm_bytes"]
# 5 measured slots x 1536 instants x 48 multiply-adds per frame
res["truepeak_batch"]["multiply_adds_per_s"] = N * 5 * 1536 * 48 / (res["truepeak_batch"]["median_ms"] * 1e-3)
print(json.dumps(res))
eng.close()
