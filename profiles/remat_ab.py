#!/usr/bin/env python3
"""Stereo encoder, rematrixing off against on (ac3mi_set_encode_rematrix): encode-call time per 65 536 frames by batch
shape, `python profiles/remat_ab.py [--once]`.  Content: correlated stereo (a shared bed, a small independent part, block
envelopes).  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python profiles/remat_ab.py --once` (three
65 536 x 1 calls per mode) and compare enc_mdct_kernel<false, false> with enc_mdct_kernel<false, true>."""
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
enc = pkg.EncodeDesc(48000, 192000, 2)
N = 65536
g = torch.Generator(device=dev).manual_seed(99)
t = torch.arange(1536, device=dev, dtype=torch.float32)
ph = torch.rand((N, 1, 1), device=dev, generator=g) * 6.28
bed = 8000.0 * torch.sin(ph + 0.02 * t[None, :, None]) + (torch.rand((N, 1536, 1), device=dev, generator=g) - 0.5) * 4096
pcm = bed + (torch.rand((N, 1536, 2), device=dev, generator=g) - 0.5) * 512
env = torch.where(torch.rand((N, 3, 1, 1), device=dev, generator=g) < 0.5, 1.0, 1.0 / 32)
pcm = (pcm.reshape(N, 3, 512, 2) * env).reshape(N, 1536, 2).round().clamp(-32768, 32767).to(torch.int16).contiguous()
for mode in (0, 1):
    eng.set_encode_rematrix(mode)
    out = []
    for S in ((65536,) if once else (65536, 8192, 1024, 128)):
        F = N // S
        x = pcm.reshape(S, F, 1536, 2)
        last = torch.zeros((S, 2, 256), dtype=torch.int16, device=dev)
        csnr = torch.full((S,), 40, dtype=torch.int32, device=dev)
        frames = torch.zeros((S, F, (enc.frame_bytes() + 3) & ~3), dtype=torch.uint8, device=dev)
        best = 1e9
        for it in range(3 if once else 4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.encode_batch(enc, x, (0, 1), last, csnr, out=frames)
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        out.append("%d x %d: %.2f ms" % (S, F, best * 1e3))
    print("rematrix %d:" % mode, " | ".join(out))
eng.set_encode_rematrix(0)
eng.close()
