// sync_rule.h — a52_syncinfo's rule on the head of an AC-3 frame (parse.c:86-129; A/52 5.3.1, 5.4.1), stated once: which heads
// are refused, the frame's size, halfrate, and where lfeon lies behind acmod.  Every reader of a frame's head calls this
// file, each with its own way of getting at the bytes: the decoder's front ends (decode_common.h: frame_own_bytes), crc.hip,
// bsi.hip, the frame scan (scan_rule.h, scan.hip) and the host's ac3mi_syncinfo and encoder set-up (capi.hip).
// Plain C++: compiles without HIP (scan_rule.h and the sanitiser programs of tests/ include it).
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace ac3mi {

// kbit/s of frmsizecod >> 1 = 0..18: 32 40 48 56, 64 80 96 112, ... 256 320 384 448 (four steps to an octave), then 512 576 640
// (arithmetic, not a table: one definition serves the host and the device, and the kernels need no load for it)
__host__ __device__ inline uint32_t sync_kbps(uint32_t i) { return i < 16u ? (4u + (i & 3u)) << (3u + (i >> 2)) : 64u * (i - 8u); }

// the frame's size in bytes from byte 4 = fscod << 6 | frmsizecod (128..3840, always even); 0: refused (frmsizecod >= 38, fscod 3)
__host__ __device__ inline uint32_t sync_frame_bytes(uint32_t b4)
{
    const uint32_t code = b4 & 63u, fscod = (b4 >> 6) & 3u;
    if (code >= 38u || fscod == 3u) return 0;
    const uint32_t rate = sync_kbps(code >> 1);
    return fscod == 0 ? 4 * rate : fscod == 1 ? 2 * (320 * rate / 147 + (code & 1u)) : 6 * rate;
}

// the test on (bytes 0-1 as a big-endian word, byte 4, byte 5): sync word, bsid < 12, and a byte 4 that has a size
__host__ __device__ inline bool sync_header_ok(uint32_t sync, uint32_t b4, uint32_t b5)
{
    return sync == 0x0b77u && b5 < 0x60u && sync_frame_bytes(b4) != 0;
}

// the same test on w0 = bytes 0-3, w1 = bytes 4-7, each little-endian (as a dword load gives them), in masks alone: the
// scan kernel's search runs it on 63 x 16 positions a round.  Bytes 2-3 and 6-7 are not looked at
__host__ __device__ inline bool sync_header_ok_le(uint32_t w0, uint32_t w1)
{
    return (w0 & 0xffffu) == 0x770bu && (w1 & 0xff00u) < 0x6000u && (w1 & 63u) < 38u && (w1 & 0xc0u) != 0xc0u;
}

// full-bandwidth channels of an acmod (A/52 table 5.8) and of liba52's three output configurations behind them (8 and 9:
// one programme of dual mono, 10: Dolby surround stereo); the decoder's field lists have their own table (dec_syntax.h)
__host__ __device__ inline int sync_nfchans(int cfg)
{
    constexpr uint8_t n[11] = {2, 1, 2, 3, 3, 4, 4, 5, 1, 1, 2};
    return n[cfg];
}

__host__ __device__ inline int sync_halfrate(int bsid) { return bsid < 9 ? 0 : bsid - 8; }

// lfeon's place in bytes 6-7 taken as a 16-bit word, counted from the word's top bit: behind acmod and the two-bit cmixlev,
// surmixlev and dsurmod that acmod sends
__host__ __device__ inline int sync_lfeon_pos(int acmod)
{
    return 3 + (((acmod & 1) && acmod != 1) ? 2 : 0) + ((acmod & 4) ? 2 : 0) + (acmod == 2 ? 2 : 0);
}

}  // namespace ac3mi
