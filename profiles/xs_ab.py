#!/usr/bin/env python3
"""Encoder, exponent strategies by the reference's rule against by cost (ac3mi_set_encode_exp_strategy 0 / 1): call time
per 65 536 one-frame 5.1 streams at 384 kb/s, for the encode call and for the transcode call (its input: the same PCM encoded
in mode 0), the two modes alternating in one process, best of the runs.  `python profiles/xs_ab.py [--once]`.  Kernel times:
run it under `rocprofv3 --kernel-trace --stats -- python profiles/xs_ab.py --once` and compare enc_mdct_kernel<..., false>
with <..., true> (the transcode's encode side runs the same kernels)."""
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
N, nch, rate, chmap = 65536, 6, 384000, (0, 2, 1, 4, 5, 3)
g = torch.Generator(device=dev).manual_seed(99)
t = torch.arange(1536, device=dev, dtype=torch.float32)
ph = torch.rand((N, 1, 1), device=dev, generator=g) * 6.28
bed = 6000.0 * torch.sin(ph + 0.02 * t[None, :, None]) + 3000.0 * torch.sin(2 * ph + 0.31 * t[None, :, None])
bed = bed + (torch.rand((N, 1536, 1), device=dev, generator=g) - 0.5) * 4096
gains = 0.4 + 0.6 * torch.rand((N, 1, nch), device=dev, generator=g)
pcm = (bed * gains + (torch.rand((N, 1536, nch), device=dev, generator=g) - 0.5) * 512).round().clamp(-32768, 32767)
x = pcm.to(torch.int16).contiguous().reshape(N, 1, 1536, nch)

enc = pkg.EncodeDesc(48000, rate, nch)
fb = enc.frame_bytes()
stride = (fb + 3) & ~3
src = torch.zeros((N, 1, stride), dtype=torch.uint8, device=dev)
eng.encode_batch(enc, x, chmap, torch.zeros((N, nch, 256), dtype=torch.int16, device=dev),
                 torch.full((N,), 40, dtype=torch.int32, device=dev), out=src)
dec = pkg.DecodeDesc(flags=7 | 16 | 32, level=1.0, bias=384.0, dynrng=1, acmod=7, lfeon=1, frame_bytes=fb)
frames = torch.zeros((N, 1, stride), dtype=torch.uint8, device=dev)

best = {}
for it in range(2 if once else 5):
    for mode in (0, 1):
        eng.set_encode_exp_strategy(mode)
        for call in ("encode", "transcode"):
            last = torch.zeros((N, nch, 256), dtype=torch.int16, device=dev)
            csnr = torch.full((N,), 40, dtype=torch.int32, device=dev)
            if call == "transcode":
                delay = torch.zeros((N, nch, 128), dtype=torch.float32, device=dev)
                lfsr = torch.ones((N,), dtype=torch.int16, device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if call == "encode":
                eng.encode_batch(enc, x, chmap, last, csnr, out=frames)
            else:
                eng.transcode_batch(dec, enc, src, delay, lfsr, chmap, last, csnr, out=frames)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best[(call, mode)] = min(best.get((call, mode), 1e9), dt)
eng.set_encode_exp_strategy(0)
for call in ("encode", "transcode"):
    print("5.1 384 kb/s, %d one-frame streams, %s call: mode 0 %.3f ms, mode 1 %.3f ms" % (N, call, best[(call, 0)] * 1e3,
                                                                                             best[(call, 1)] * 1e3))
eng.close()
