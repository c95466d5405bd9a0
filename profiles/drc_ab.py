#!/usr/bin/env python3
"""Encoder, dynamic range control off against on (ac3mi_set_encode_drc): encode-call time per 65 536 one-frame 5.1 streams
at 384 kb/s, profile 0 against profile 1 (dialnorm 24), `python profiles/drc_ab.py [--once]`.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python profiles/drc_ab.py --once` (three calls per case) and compare
enc_drc_gain_kernel / enc_drc_smooth_kernel and the DRC / MD variants of the search and packer with the rest."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench

once = "--once" in sys.argv
pkg = bench.importlib_pkg()
dev = torch.device("cuda:0")
eng = pkg.Engine(0)
N, nch = 65536, 6
g = torch.Generator(device=dev).manual_seed(99)
t = torch.arange(1536, device=dev, dtype=torch.float32)
ph = torch.rand((N, 1, 1), device=dev, generator=g) * 6.28
bed = 6000.0 * torch.sin(ph + 0.02 * t[None, :, None]) + 3000.0 * torch.sin(2 * ph + 0.31 * t[None, :, None])
bed = bed + (torch.rand((N, 1536, 1), device=dev, generator=g) - 0.5) * 4096
gains = 0.4 + 0.6 * torch.rand((N, 1, nch), device=dev, generator=g)
pcm = (bed * gains + (torch.rand((N, 1536, nch), device=dev, generator=g) - 0.5) * 512).round().clamp(-32768, 32767)
x = pcm.to(torch.int16).reshape(N, 1, 1536, nch).contiguous()
enc = pkg.EncodeDesc(48000, 384000, nch)
chmap = (0, 2, 1, 4, 5, 3)
state = torch.zeros((N,), dtype=torch.int32, device=dev)
res = {}
for profile in (0, 1, 0, 1):
    eng.set_encode_metadata(dialnorm=24) if profile else eng.set_encode_metadata()
    eng.set_encode_drc(profile, state if profile else None)
    last = torch.zeros((N, nch, 256), dtype=torch.int16, device=dev)
    csnr = torch.full((N,), 40, dtype=torch.int32, device=dev)
    frames = torch.zeros((N, 1, (enc.frame_bytes() + 3) & ~3), dtype=torch.uint8, device=dev)
    best = 1e9
    for it in range(3 if once else 6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.encode_batch(enc, x, chmap, last, csnr, out=frames)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    res[profile] = min(res.get(profile, 1e9), best)
eng.set_encode_drc(0)
eng.set_encode_metadata()
for profile in (0, 1):
    print("5.1 384 kb/s, 65 536 one-frame streams, DRC profile %d: %.3f ms" % (profile, res[profile] * 1e3))
print("DRC on / off: %.3f" % (res[1] / res[0]))
eng.close()
