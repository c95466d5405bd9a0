#!/usr/bin/env python3
"""Encoder layouts (ac3mi_set_encode_layout): call time per 65 536 one-frame streams of 2/0+LFE with rematrixing against 3/0
(three coded channels each, 192 kb/s), and of dual mono against 2/0 (192 kb/s), best of the runs.
`python profiles/layout_cost.py [--once] [CASE ...]`, CASE one of 21r 30 0 20 (default all).  Kernel times: run one case per
process under `rocprofv3 --kernel-trace --stats -- python profiles/layout_cost.py --once 21r`."""
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
N, rate = 65536, 192000
CASES = {"21r": (2, 1, 1), "30": (3, 0, 0), "0": (0, 0, 0), "20": (2, 0, 0)}      # acmod, lfeon, rematrixing
names = [a for a in sys.argv[1:] if a in CASES] or list(CASES)
g = torch.Generator(device=dev).manual_seed(99)
t = torch.arange(1536, device=dev, dtype=torch.float32)
ph = torch.rand((N, 1, 1), device=dev, generator=g) * 6.28
bed = 6000.0 * torch.sin(ph + 0.02 * t[None, :, None]) + 3000.0 * torch.sin(2 * ph + 0.31 * t[None, :, None])
bed = bed + (torch.rand((N, 1536, 1), device=dev, generator=g) - 0.5) * 4096

best = {}
for it in range(2 if once else 5):
    for name in names:
        acmod, lfeon, remat = CASES[name]
        nch = (2, 1, 2, 3, 3, 4, 4, 5)[acmod] + lfeon
        gains = 0.4 + 0.6 * torch.rand((N, 1, nch), device=dev, generator=g)
        pcm = (bed * gains + (torch.rand((N, 1536, nch), device=dev, generator=g) - 0.5) * 512).round().clamp(-32768, 32767)
        x = pcm.to(torch.int16).contiguous().reshape(N, 1, 1536, nch)
        enc = pkg.EncodeDesc(48000, rate, nch)
        frames = torch.zeros((N, 1, (enc.frame_bytes() + 3) & ~3), dtype=torch.uint8, device=dev)
        last = torch.zeros((N, nch, 256), dtype=torch.int16, device=dev)
        csnr = torch.full((N,), 40, dtype=torch.int32, device=dev)
        eng.set_encode_layout(1, acmod, lfeon)
        eng.set_encode_rematrix(remat)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.encode_batch(enc, x, tuple(range(nch)), last, csnr, out=frames)
        torch.cuda.synchronize()
        best[name] = min(best.get(name, 1e9), time.perf_counter() - t0)
        eng.set_encode_layout(0)
        eng.set_encode_rematrix(0)
LABEL = {"21r": "2/0+LFE with rematrixing", "30": "3/0", "0": "dual mono", "20": "2/0"}
for name in names:
    print("%s, %d one-frame streams at %d kb/s: encode call %.3f ms" % (LABEL[name], N, rate // 1000, best[name] * 1e3))
eng.close()
