#!/usr/bin/env python3
"""The sample-rate converter (ac3mi_resample_batch) on 65 536 one-frame streams - 5.1 and 2/0 at 44.1 -> 48 kHz, 5.1 at
32 -> 44.1 kHz (the largest table, 441 phases) - beside three yardsticks taken in the same run on the same 5.1 buffer:
ac3mi_limit_batch and ac3mi_truepeak_batch, the other two polyphase stages, and ac3mi_probe_copy_rate scaled to the bytes the
converter reads and writes (a bare copy).  A call's shape depends on the streams' age, so every pass starts from the same
states, put back outside the timed region: new streams (`first`: one frame in, one out, nothing pending before) and streams
that have had five frames (`sixth`: the pending instants of the state move to the output's head, new ones take their place).
`python profiles/resample_ab.py [--streams N] [--passes P]`.
Times are ac3mi_timer_* (HIP events on the engine's stream) around one call, warm; every case is timed P times with the cases
interleaved and reported as median with min / max.  Prints one JSON line.
Kernel times: `rocprofv3 --kernel-trace --stats -- python profiles/resample_ab.py --passes 3` and look for resample_kernel."""
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
N = args.streams
g = torch.Generator(device=dev).manual_seed(99)                     # profiles/truepeak_ab.py's content
t = torch.arange(1536, device=dev, dtype=torch.float32)
ph = torch.rand((N, 1, 1), device=dev, generator=g) * 6.28
bed = 6000.0 * torch.sin(ph + 0.02 * t[None, :, None]) + 3000.0 * torch.sin(2 * ph + 0.31 * t[None, :, None])
bed = bed + (torch.rand((N, 1536, 1), device=dev, generator=g) - 0.5) * 4096
gains = 0.4 + 0.6 * torch.rand((N, 1, 6), device=dev, generator=g)
pcm = (bed * gains + (torch.rand((N, 1536, 6), device=dev, generator=g) - 0.5) * 512).round().clamp(-32768, 32767)
x6 = pcm.to(torch.int16).reshape(N, 1, 1536, 6).contiguous()
x2 = x6[..., :2].contiguous()
del pcm, bed
nb = pkg.resample_state_bytes()
state = torch.zeros((N, nb), dtype=torch.uint8, device=dev)
status = torch.zeros((N,), dtype=torch.int32, device=dev)


def aged(pair, x, calls):
    """the states of streams that have had `calls` one-frame calls of x, and what the next call takes"""
    state.zero_()
    n_in = f_out = 0
    for _ in range(calls):
        of, _ = pkg.resample_plan(*pair, n_in, f_out, 1)
        eng.resample_batch(pair, x, of, state, status=status)
        n_in, f_out = n_in + 1536, f_out + of
    eng.sync()
    assert int(status.abs().max()) == 0
    return state.clone(), pkg.resample_plan(*pair, n_in, f_out, 1)[0]


UP, BIG = (44100, 48000), (32000, 44100)
shapes = {"resample_441_48_51_first": (UP, x6, 0), "resample_441_48_51_sixth": (UP, x6, 5), "resample_441_48_20_first": (UP, x2, 0),
          "resample_32_441_51_first": (BIG, x6, 0)}
start, outs, cases = {}, {}, {}
for k, (pair, x, calls) in shapes.items():
    start[k], of = aged(pair, x, calls)
    assert of == 1
    outs[k] = torch.empty_like(x)
    cases[k] = (lambda pair=pair, x=x, k=k: eng.resample_batch(pair, x, 1, state, outs[k], status, wait_torch=False))

roles = pkg.loudness_roles(7 | 16)
lim_state = torch.zeros((N, pkg.limit_state_bytes()), dtype=torch.uint8, device=dev)
lim_out = torch.empty_like(x6)
tp_state = torch.zeros((N, pkg.truepeak_state_bytes()), dtype=torch.uint8, device=dev)
ceiling, step = pkg.truepeak_ceiling(-1.0), pkg.limit_release_step(48000, 100.0)
cases["limit_batch"] = lambda: eng.limit_batch(roles, ceiling, step, x6, lim_state, lim_out, wait_torch=False)
cases["truepeak_batch"] = lambda: eng.truepeak_batch(roles, x6, tp_state, wait_torch=False)


def timed(k):
    if k in start:
        state.copy_(start[k])                           # outside the timed region
        torch.cuda.synchronize(dev)
    eng.timer_start()
    cases[k]()
    return eng.timer_stop()


def stats(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "passes": len(xs)}


for _ in range(3):                                      # warm: every kernel of every case has run, every table is on the device
    for k in cases:
        timed(k)
eng.sync()
tm = {k: [] for k in cases}
for _ in range(args.passes):
    for k in cases:
        tm[k].append(timed(k))
eng.sync()
assert int(status.abs().max()) == 0

copy_gbs = eng.probe_copy_rate(1 << 30)
res = {"streams": N, "frames_per_stream": 1, "state_bytes": state.numel(), "device": torch.cuda.get_device_name(0),
       "copy_probe_gb_per_s_read_plus_written": copy_gbs}
for k in cases:
    res[k] = stats(tm[k])
    if k in shapes:
        nbytes = shapes[k][1].numel() * 2 + outs[k].numel() * 2     # the PCM read and written; the state's history and pending come on top
        res[k]["pcm_bytes_read_and_written"] = nbytes
        res[k]["copy_probe_ms_for_those_bytes"] = nbytes / (copy_gbs * 1e9) * 1e3
        res[k]["over_copy_probe_time"] = res[k]["median_ms"] / res[k]["copy_probe_ms_for_those_bytes"]
        res[k]["ns_per_frame"] = res[k]["median_ms"] * 1e6 / N
print(json.dumps(res))
eng.close()
