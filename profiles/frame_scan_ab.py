#!/usr/bin/env python3
"""Finding frames in device byte streams (ac3mi_frame_scan_batch mode 0 / 1, ac3mi_frame_gather_batch) against the check that
reads the same bytes (ac3mi_crc_check_batch on the gathered frames), on 65 536 streams of four clean 5.1 frames at 384 kb/s,
and on the same streams with 1 KiB of random bytes in front, so that the cooperative search runs:
`python profiles/frame_scan_ab.py [--frames N] [--passes P]` (N = streams).
Times are ac3mi_timer_* (HIP events on the engine's stream) around one call, warm; every case is timed P times with the cases
interleaved and reported as median with min / max.  Read rates stand against ac3mi_probe_copy_rate (a bare copy moves read +
written bytes; the scan only reads, the gather reads and writes).  Prints one JSON line.
Kernel times: `rocprofv3 --kernel-trace --stats -- python profiles/frame_scan_ab.py --passes 3` and look for
frame_scan_kernel / frame_gather_kernel."""
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
S, F, JUNK = args.frames, 4, 1024
C = bench.Content(pkg, eng, dev, S, 0)                   # seeded PCM -> AC-3 frames, as bench.py's legs use them
fb = C.fb
one = C.frames.reshape(S, fb)
idx = torch.arange(S, device=dev)
clean = torch.stack([one[(idx + 7919 * j) % S] for j in range(F)], dim=1).reshape(S, F * fb).contiguous()
junk = torch.randint(0, 256, (S, JUNK), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
junk[junk == 0x0b] = 0x0c                                # no sync word in front of the frames: every stream lists its four
dirty = torch.cat([junk, clean], dim=1).contiguous()
assert clean.shape[1] % 16 == 0 and dirty.shape[1] % 16 == 0
len_clean = torch.full((S,), F * fb, dtype=torch.int32, device=dev)
len_dirty = torch.full((S,), JUNK + F * fb, dtype=torch.int32, device=dev)
refs = torch.zeros((S, F, 8), dtype=torch.uint8, device=dev)
info = torch.zeros((S, 24), dtype=torch.uint8, device=dev)
refs_d, info_d = torch.zeros_like(refs), torch.zeros_like(info)
frames = torch.zeros((S, F, fb), dtype=torch.uint8, device=dev)
verdict = torch.zeros((S, F), dtype=torch.uint8, device=dev)
torch.cuda.synchronize(dev)

cases = {
    "scan_mode0": lambda: eng.frame_scan_batch(clean, len_clean, 0, F, refs=refs, info=info, wait_torch=False),
    "scan_mode1": lambda: eng.frame_scan_batch(clean, len_clean, 1, F, refs=refs, info=info, wait_torch=False),
    "gather": lambda: eng.frame_gather_batch(clean, refs, info, F, fb, frame_stride=fb, out=frames, wait_torch=False),
    "crc_check_batch": lambda: eng.crc_check_batch(frames, fb, out=verdict, wait_torch=False),
    "scan_mode0_dirty": lambda: eng.frame_scan_batch(dirty, len_dirty, 0, F, refs=refs_d, info=info_d, wait_torch=False),
    "scan_mode1_dirty": lambda: eng.frame_scan_batch(dirty, len_dirty, 1, F, refs=refs_d, info=info_d, wait_torch=False),
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
t = {k: [] for k in cases}
for _ in range(args.passes):
    for k, fn in cases.items():
        t[k].append(timed(fn))
eng.sync()
dt = pkg.capi.scan_info_dtype()
for arr, skipped in ((info, 0), (info_d, JUNK)):
    rec = arr.cpu().numpy().view(dt)[..., 0]
    assert (rec["n_frames"] == F).all() and (rec["skipped"] == skipped).all() and (rec["consumed"] == skipped + F * fb).all()
assert torch.equal(frames.reshape(S, F * fb), clean) and int(verdict.max().item()) == 0

copy_gbs = eng.probe_copy_rate(1 << 30)
res = {"streams": S, "frames_per_stream": F, "frame_bytes": fb, "junk_bytes": JUNK, "device": torch.cuda.get_device_name(0),
       "copy_probe_gb_per_s_read_plus_written": copy_gbs}
nbytes = {"scan_mode0": S * F * fb, "scan_mode1": S * F * fb, "gather": S * F * fb, "crc_check_batch": S * F * fb,
          "scan_mode0_dirty": S * (JUNK + F * fb), "scan_mode1_dirty": S * (JUNK + F * fb)}
for k in cases:
    r = stats(t[k])
    r["stream_bytes"] = nbytes[k]
    r["stream_gb_per_s"] = nbytes[k] / (r["median_ms"] * 1e-3) / 1e9
    r["stream_rate_over_copy_probe"] = r["stream_gb_per_s"] / copy_gbs
    r["frames_per_s"] = S * F / (r["median_ms"] * 1e-3)
    r["ns_per_frame"] = r["median_ms"] * 1e6 / (S * F)   # the scans: the cost of a hop of the serial walk, all streams in flight
    res[k] = r
res["mode1_over_crc_check_plus_gather"] = res["scan_mode1"]["median_ms"] / (res["crc_check_batch"]["median_ms"] + res["gather"]["median_ms"])
res["mode1_over_crc_check"] = res["scan_mode1"]["median_ms"] / res["crc_check_batch"]["median_ms"]
res["search_ms_mode0"] = res["scan_mode0_dirty"]["median_ms"] - res["scan_mode0"]["median_ms"]
print(json.dumps(res))
eng.close()
