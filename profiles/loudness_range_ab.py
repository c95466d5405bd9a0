#!/usr/bin/env python3
"""The loudness range meter (ac3mi_loudness_range_batch, ac3mi_loudness_range_read_batch) beside the plain BS.1770 meter it
rides on (ac3mi_loudness_batch, ac3mi_loudness_read_batch: the yardsticks), on 65 536 one-frame 5.1 streams at 48 kHz (1.2 GB
of s16 PCM, profiles/loudness_ab.py's content).
`python profiles/loudness_range_ab.py [--streams N] [--passes P]`.
Times are ac3mi_timer_* (HIP events on the engine's stream) around one call, warm; every case is timed P times with the cases
interleaved and reported as median with min / max.  One-frame streams close a hop in one call out of three (a hop is 3.125
frames), and a 3 s block only from the 30th hop on: the states are carried from call to call, so after the warm calls and
the passes every stream has formed blocks.  Prints one JSON line.
Kernel times: `rocprofv3 --kernel-trace --stats -- python profiles/loudness_range_ab.py --passes 3` and look for
loudness_kernel / loudness_range_read_kernel."""
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
ap.add_argument("--warm", type=int, default=96, help="warm calls per case: 94 one-frame calls close the 30th hop")
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
nb, nr = pkg.loudness_state_bytes(), pkg.loudness_range_state_bytes()
plain = torch.zeros((N, nb), dtype=torch.uint8, device=dev)
plain_off, state, state_off = torch.zeros_like(plain), torch.zeros_like(plain), torch.zeros_like(plain)
rstate = torch.zeros((N, nr), dtype=torch.uint8, device=dev)
rstate_off = torch.zeros_like(rstate)
results = torch.zeros((N, 40), dtype=torch.uint8, device=dev)
rresults = torch.zeros((N, 48), dtype=torch.uint8, device=dev)
torch.cuda.synchronize(dev)

cases = {
    "loudness_batch": lambda: eng.loudness_batch(48000, roles, x, plain, wait_torch=False),
    "loudness_batch_unaligned": lambda: eng.loudness_batch(48000, roles, x_off, plain_off, wait_torch=False),
    "loudness_range_batch": lambda: eng.loudness_range_batch(48000, roles, x, state, rstate, wait_torch=False),
    "loudness_range_batch_unaligned": lambda: eng.loudness_range_batch(48000, roles, x_off, state_off, rstate_off, wait_torch=False),
    "loudness_read_batch": lambda: eng.loudness_read_batch(plain, out=results, wait_torch=False),
    "loudness_range_read_batch": lambda: eng.loudness_range_read_batch(rstate, out=rresults, wait_torch=False),
}


def timed(fn):
    eng.timer_start()
    fn()
    return eng.timer_stop()


def stats(xs):
    return {"median_ms": statistics.median(xs), "mean_ms": statistics.fmean(xs), "min_ms": min(xs), "max_ms": max(xs), "passes": len(xs)}


for _ in range(max(3, args.warm)):                      # warm: every kernel has run, and every stream forms 3 s blocks
    for fn in cases.values():
        fn()
eng.sync()
tm = {k: [] for k in cases}
for _ in range(args.passes):
    for k, fn in cases.items():
        tm[k].append(timed(fn))
eng.sync()
assert torch.equal(plain, plain_off) and torch.equal(state, plain), "the range pass leaves another loudness state than the plain meter"
assert torch.equal(state, state_off) and torch.equal(rstate, rstate_off), "the two load paths differ"
rr = rresults.cpu().numpy().view(pkg.capi.loudness_range_result_dtype())[:, 0]

nbytes = x.numel() * 2
res = {"streams": N, "frames_per_stream": 1, "channels": nch, "sample_rate": 48000, "pcm_bytes": nbytes, "state_bytes": plain.numel(),
       "range_state_bytes": rstate.numel(), "device": torch.cuda.get_device_name(0), "calls_per_stream": max(3, args.warm) + args.passes,
       "blocks_per_stream": int(rr["blocks"].min()), "lra_tenths_max": int(rr["lra_tenths"].max())}
for k in cases:
    res[k] = stats(tm[k])
for k in ("loudness_batch", "loudness_batch_unaligned", "loudness_range_batch", "loudness_range_batch_unaligned"):
    res[k]["pcm_gb_per_s"] = nbytes / (res[k]["median_ms"] * 1e-3) / 1e9
    res[k]["ns_per_frame"] = res[k]["median_ms"] * 1e6 / N
res["range_over_plain"] = res["loudness_range_batch"]["median_ms"] / res["loudness_batch"]["median_ms"]
res["range_over_plain_mean"] = res["loudness_range_batch"]["mean_ms"] / res["loudness_batch"]["mean_ms"]   # (a hop closes in one pass of three)
res["range_unaligned_over_plain_unaligned"] = res["loudness_range_batch_unaligned"]["median_ms"] / res["loudness_batch_unaligned"]["median_ms"]
res["range_read_over_read"] = res["loudness_range_read_batch"]["median_ms"] / res["loudness_read_batch"]["median_ms"]
print(json.dumps(res))
eng.close()
