#!/usr/bin/env python3
"""Encoder, audio bandwidth off against on (ac3mi_set_encode_bandwidth): encode-call time per 65 536 one-frame streams for
5.1 at 384 kb/s (mode 0 against mode 1, chbwcod 32) and 2/0 at 96 kb/s (mode 0 against mode 2, chbwcod 25 there),
`python profiles/bw_ab.py [--once]`.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python
profiles/bw_ab.py --once` (three calls per case) and compare the encode kernels (5.1 band-limited packs with
enc_packf_kernel<true, false, true>, the 5.1 shape with the run-time nbc)."""
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
N = 65536
g = torch.Generator(device=dev).manual_seed(99)
t = torch.arange(1536, device=dev, dtype=torch.float32)


def content(nch):
    ph = torch.rand((N, 1, 1), device=dev, generator=g) * 6.28
    bed = 6000.0 * torch.sin(ph + 0.02 * t[None, :, None]) + 3000.0 * torch.sin(2 * ph + 0.31 * t[None, :, None])
    bed = bed + (torch.rand((N, 1536, 1), device=dev, generator=g) - 0.5) * 4096
    gains = 0.4 + 0.6 * torch.rand((N, 1, nch), device=dev, generator=g)
    pcm = bed * gains + (torch.rand((N, 1536, nch), device=dev, generator=g) - 0.5) * 512
    return pcm.round().clamp(-32768, 32767).to(torch.int16).contiguous()


for name, nch, rate, chmap, modes in (("5.1 384 kb/s", 6, 384000, (0, 2, 1, 4, 5, 3), ((0, 50), (1, 32))),
                                       ("2/0 96 kb/s", 2, 96000, (0, 1), ((0, 50), (2, 0)))):
    enc = pkg.EncodeDesc(48000, rate, nch)
    pcm = content(nch)
    x = pcm.reshape(N, 1, 1536, nch)
    for mode, c in modes:
        eng.set_encode_bandwidth(mode, c)
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
        what = {0: "", 1: " (chbwcod %d)" % c, 2: " (chbwcod by the table)"}[mode]
        print("%s, bandwidth mode %d%s: %.3f ms" % (name, mode, what, best * 1e3))
    eng.set_encode_bandwidth(0)
eng.close()
