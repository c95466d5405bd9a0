#!/usr/bin/env python3
"""5.1 encoder, channel coupling off against on (ac3mi_set_encode_coupling, begf 0): encode-call time per 65 536 frames by
batch shape, `python profiles/cpl_ab.py [--once]`.  Content: one bed at per-channel gains plus small independent parts,
so that most frames couple.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python profiles/cpl_ab.py
--once` (three 65 536 x 1 calls per mode) and compare the encode kernels of the two modes (mode 1 adds enc_cpl_kernel and
packs with enc_packf_kernel<false>)."""
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
enc = pkg.EncodeDesc(48000, 384000, 6)
chmap = (0, 2, 1, 4, 5, 3)
N = 65536
g = torch.Generator(device=dev).manual_seed(99)
t = torch.arange(1536, device=dev, dtype=torch.float32)
ph = torch.rand((N, 1, 1), device=dev, generator=g) * 6.28
bed = 6000.0 * torch.sin(ph + 0.02 * t[None, :, None]) + 3000.0 * torch.sin(2 * ph + 0.31 * t[None, :, None])
bed = bed + (torch.rand((N, 1536, 1), device=dev, generator=g) - 0.5) * 4096
gains = 0.4 + 0.6 * torch.rand((N, 1, 6), device=dev, generator=g)
pcm = bed * gains + (torch.rand((N, 1536, 6), device=dev, generator=g) - 0.5) * 512
pcm = pcm.round().clamp(-32768, 32767).to(torch.int16).contiguous()
for mode in (0, 1):
    eng.set_encode_coupling(mode, 0)
    out = []
    for S in ((65536,) if once else (65536, 8192, 1024, 128)):
        F = N // S
        x = pcm.reshape(S, F, 1536, 6)
        last = torch.zeros((S, 6, 256), dtype=torch.int16, device=dev)
        csnr = torch.full((S,), 40, dtype=torch.int32, device=dev)
        frames = torch.zeros((S, F, (enc.frame_bytes() + 3) & ~3), dtype=torch.uint8, device=dev)
        best = 1e9
        for it in range(3 if once else 4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.encode_batch(enc, x, chmap, last, csnr, out=frames)
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        out.append("%d x %d: %.2f ms" % (S, F, best * 1e3))
    print("coupling %d:" % mode, " | ".join(out))
eng.set_encode_coupling(0, 0)
eng.close()
