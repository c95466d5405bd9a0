#!/usr/bin/env python3
"""CRC verification off against on (ac3mi_set_decode_crc 0 / 1 / 2) and the check alone (ac3mi_crc_check_batch), on 65 536
one-frame 5.1 streams at 384 kb/s, intact input: `python profiles/crc_check_ab.py [--frames N] [--passes P]`.
Times are ac3mi_timer_* (HIP events on the engine's stream) around one call, warm; every case is timed P times with the
cases interleaved (0, 1, 2, 0, 1, 2, ...) and reported as median with min / max.  The check's read rate stands against
ac3mi_probe_copy_rate (a bare copy moves read + written bytes; the check only reads).  Prints one JSON line.
Kernel times: `rocprofv3 --kernel-trace --stats -- python profiles/crc_check_ab.py --passes 3` and look for crc_kernel."""
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
verdict = torch.zeros((S, 1), dtype=torch.uint8, device=dev)
out16 = torch.empty((S, 1, 6, 256, 6), dtype=torch.int16, device=dev)
delay = torch.zeros((S, 6, 128), dtype=torch.float32, device=dev)
lfsr = torch.ones((S,), dtype=torch.int16, device=dev)
status = torch.zeros((S, 1), dtype=torch.int32, device=dev)
torch.cuda.synchronize(dev)


def check():
    eng.crc_check_batch(frames, C.fb, out=verdict, wait_torch=False)


def decode():
    eng.decode_s16_batch(C.dec, frames, delay, lfsr, out=out16, status=status, wait_torch=False)


def transcode():
    C.transcode()


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
    for mode in (0, 1, 2):
        eng.set_decode_crc(mode)
        decode()
        C.reset_transcode()
        transcode()
    check()
eng.sync()
t = {("check",): [], **{("decode_s16", m): [] for m in (0, 1, 2)}, **{("transcode", m): [] for m in (0, 1, 2)}}
for _ in range(args.passes):
    t[("check",)].append(timed(check))
    for mode in (0, 1, 2):
        eng.set_decode_crc(mode)
        t[("decode_s16", mode)].append(timed(decode))
        t[("transcode", mode)].append(timed(transcode, C.reset_transcode))
eng.set_decode_crc(0)
eng.sync()
assert int(verdict.max().item()) == 0 and int((status & 0xfff).max().item()) == 0 and int((C.status_tc & 0xfff).max().item()) == 0

copy_gbs = eng.probe_copy_rate(1 << 30)
chk = stats(t[("check",)])
chk["read_bytes"] = S * C.fb
chk["read_gb_per_s"] = S * C.fb / (chk["median_ms"] * 1e-3) / 1e9
chk["copy_probe_gb_per_s_read_plus_written"] = copy_gbs
chk["read_rate_over_copy_probe"] = chk["read_gb_per_s"] / copy_gbs
res["crc_check_batch"] = chk
for leg in ("decode_s16", "transcode"):
    res[leg] = {"mode%d" % m: stats(t[(leg, m)]) for m in (0, 1, 2)}
    for m in (1, 2):
        res[leg]["mode%d_minus_mode0_ms" % m] = res[leg]["mode%d" % m]["median_ms"] - res[leg]["mode0"]["median_ms"]
print(json.dumps(res))
eng.close()
