#!/usr/bin/env python3
"""The BS.1770 meter (ac3mi_loudness_batch, ac3mi_loudness_read_batch, ac3mi_loudness_words_batch) on 65 536 one-frame 5.1
streams at 48 kHz (1.2 GB of s16 PCM), beside the one other kernel that only reads that PCM: enc_drc_gain_kernel, timed as
ac3mi_encode_batch under DRC profile 1 minus profile 0 in the same session (the difference also holds enc_drc_smooth_kernel
and the DRC variants of the search and packer, so it is an upper bound on the read).
`python profiles/loudness_ab.py [--streams N] [--passes P]`.
Times are ac3mi_timer_* (HIP events on the engine's stream) around one call, warm; every case is timed P times with the cases
interleaved and reported as median with min / max.  Read rates stand against ac3mi_probe_copy_rate (a bare copy moves read +
written bytes; the meter only reads).  Prints one JSON line.
Kernel times: `rocprofv3 --kernel-trace --stats -- python profiles/loudness_ab.py --passes 3` and look for loudness_kernel /
loudness_read_kernel / enc_drc_gain_kernel."""
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
g = torch.Generator(device=dev).manual_seed(99)                     # profiles/drc_ab.py's content
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
state = torch.zeros((N, pkg.loudness_state_bytes()), dtype=torch.uint8, device=dev)
state_off = torch.zeros_like(state)
results = torch.zeros((N, 40), dtype=torch.uint8, device=dev)
words = torch.zeros((N, 1), dtype=torch.int32, device=dev)
enc = pkg.EncodeDesc(48000, 384000, nch)
chmap = (0, 2, 1, 4, 5, 3)
drc_state = torch.zeros((N,), dtype=torch.int32, device=dev)
last = torch.zeros((N, nch, 256), dtype=torch.int16, device=dev)
csnr = torch.full((N,), 40, dtype=torch.int32, device=dev)
frames = torch.zeros((N, 1, (enc.frame_bytes() + 3) & ~3), dtype=torch.uint8, device=dev)
torch.cuda.synchronize(dev)


def encode(profile):
    eng.set_encode_metadata(dialnorm=24) if profile else eng.set_encode_metadata()
    eng.set_encode_drc(profile, drc_state if profile else None)
    eng.encode_batch(enc, x, chmap, last, csnr, out=frames, wait_torch=False)


cases = {
    "loudness_batch": lambda: eng.loudness_batch(48000, roles, x, state, wait_torch=False),
    "loudness_batch_unaligned": lambda: eng.loudness_batch(48000, roles, x_off, state_off, wait_torch=False),
    "loudness_read_batch": lambda: eng.loudness_read_batch(state, out=results, wait_torch=False),
    "loudness_words_batch": lambda: eng.loudness_words_batch(results, 1, 0, out=words, wait_torch=False),
    "encode_drc0": lambda: encode(0),
    "encode_drc1": lambda: encode(1),
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
eng.set_encode_drc(0)
eng.set_encode_metadata()
assert torch.equal(state, state_off), "the two load paths differ"

copy_gbs = eng.probe_copy_rate(1 << 30)
nbytes = x.numel() * 2
res = {"streams": N, "frames_per_stream": 1, "channels": nch, "sample_rate": 48000, "pcm_bytes": nbytes, "state_bytes": state.numel(),
       "device": torch.cuda.get_device_name(0), "copy_probe_gb_per_s_read_plus_written": copy_gbs}
for k in cases:
    res[k] = stats(tm[k])
for k in ("loudness_batch", "loudness_batch_unaligned"):
    res[k]["pcm_gb_per_s"] = nbytes / (res[k]["median_ms"] * 1e-3) / 1e9
    res[k]["pcm_rate_over_copy_probe"] = res[k]["pcm_gb_per_s"] / copy_gbs
    res[k]["ns_per_frame"] = res[k]["median_ms"] * 1e6 / N
res["loudness_read_batch"]["state_gb_per_s"] = state.numel() / (res["loudness_read_batch"]["median_ms"] * 1e-3) / 1e9
res["drc_pass_ms"] = res["encode_drc1"]["median_ms"] - res["encode_drc0"]["median_ms"]
res["drc_pass_pcm_gb_per_s"] = nbytes / (res["drc_pass_ms"] * 1e-3) / 1e9 if res["drc_pass_ms"] > 0 else None
res["loudness_over_drc_pass"] = res["loudness_batch"]["median_ms"] / res["drc_pass_ms"] if res["drc_pass_ms"] > 0 else None
print(json.dumps(res))
eng.close()
