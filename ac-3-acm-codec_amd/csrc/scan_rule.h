// scan_rule.h — the framing rule of ac3mi_frame_scan / ac3mi_frame_scan_batch (include/ac3mi.h), the part that needs no GPU:
// a52_syncinfo's header test and the frame's size on six bytes (parse.c:86-129, as crc.hip and bsi.hip restate it), one
// __host__ __device__ function that the host walk below and frame_scan_kernel (scan.hip) both call, and the host walk itself,
// stream_convert_ac3's resync rule (run_decode in stream.hip) with the two CRC sums of crc.hip in plain C.
// Plain C++: compiles without HIP (a host-only build of scan.hip for the sanitiser program of tests/frame_scan_c).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/ac3mi.h"

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace ac3mi {

// w0 = bytes 0-3 of a candidate, w1 = bytes 4-7, each little-endian (as a dword load gives them); bytes 2-3 and 6-7 are not
// looked at.  a52_syncinfo's test: sync word, bsid byte < 0x60, frmsizecod < 38, fscod != 3 (all the kernel's search needs)
__host__ __device__ inline bool scan_header_ok(uint32_t w0, uint32_t w1)
{
    return (w0 & 0xffffu) == 0x770bu && (w1 & 0xff00u) < 0x6000u && (w1 & 63u) < 38u && (w1 & 0xc0u) != 0xc0u;
}

// ... and the frame's size in bytes (128..3840, always even); 0: the test refuses the header
__host__ __device__ inline uint32_t scan_header_size(uint32_t w0, uint32_t w1)
{
    if (!scan_header_ok(w0, w1)) return 0;
    const uint32_t code = w1 & 63u, fscod = (w1 >> 6) & 3u;
    uint32_t rate;                                      // (a switch, not a table: one definition serves the host and the device)
    switch (code >> 1) {
    case 0: rate = 32; break; case 1: rate = 40; break; case 2: rate = 48; break; case 3: rate = 56; break;
    case 4: rate = 64; break; case 5: rate = 80; break; case 6: rate = 96; break; case 7: rate = 112; break;
    case 8: rate = 128; break; case 9: rate = 160; break; case 10: rate = 192; break; case 11: rate = 224; break;
    case 12: rate = 256; break; case 13: rate = 320; break; case 14: rate = 384; break; case 15: rate = 448; break;
    case 16: rate = 512; break; case 17: rate = 576; break; default: rate = 640; break;
    }
    return fscod == 0 ? 4 * rate : fscod == 1 ? 2 * (320 * rate / 147 + (code & 1u)) : 6 * rate;
}

// end of crc1's region = start of crc2's, in bytes, for a frame of `bytes` (A/52: 2 fs58, fs in 16-bit words)
__host__ __device__ inline uint32_t scan_region1_end(uint32_t bytes)
{
    const uint32_t fs = bytes >> 1;
    return 2 * ((fs >> 1) + (fs >> 3));
}

// CRC-16, x^16 + x^15 + x^2 + 1, MSB first, bit by bit from a running value (host only: the kernel sums by table)
inline uint32_t scan_crc16(const uint8_t *p, size_t n, uint32_t crc = 0)
{
    for (size_t i = 0; i < n; i++) {
        crc ^= (uint32_t)p[i] << 8;
        for (int k = 0; k < 8; k++) crc = (crc & 0x8000u) ? (((crc << 1) & 0xffffu) ^ 0x8005u) : (crc << 1);
    }
    return crc;
}

// The walk of include/ac3mi.h on host bytes.  len < 2^32, max_frames >= 1, mode 0 / 1 (the caller has checked)
inline void frame_scan_host(const uint8_t *buf, size_t len, int mode, int max_frames, ac3mi_frame_ref *refs, ac3mi_scan_info *info)
{
    auto le32 = [&](size_t p) { return (uint32_t)buf[p] | (uint32_t)buf[p + 1] << 8 | (uint32_t)buf[p + 2] << 16 | (uint32_t)buf[p + 3] << 24; };
    size_t p = 0;
    uint32_t n = 0, skipped = 0, rejected = 0, flags = 0;
    while (p + 8 <= len && n < (uint32_t)max_frames) {
        const uint32_t fs = scan_header_size(le32(p), le32(p + 4));
        if (fs) {
            if (p + fs > len) {
                flags |= AC3MI_SCAN_INCOMPLETE;
                break;
            }
            const uint32_t e1 = scan_region1_end(fs);
            if (mode == 0 || (scan_crc16(buf + p + 2, e1 - 2) == 0 && scan_crc16(buf + p + e1, (fs & ~1u) - e1) == 0)) {
                refs[n].offset = (uint32_t)p;
                refs[n].bytes = (uint16_t)fs;
                refs[n].sizecod = buf[p + 4];
                refs[n].reserved = 0;
                n++;
                p += fs;
                continue;
            }
            rejected++;
        }
        p++;
        skipped++;
    }
    if (n == (uint32_t)max_frames && p + 8 <= len) flags |= AC3MI_SCAN_CAPPED;
    info->n_frames = n;
    info->consumed = (uint32_t)p;
    info->skipped = skipped;
    info->rejected = rejected;
    info->flags = flags;
    info->reserved = 0;
}

}  // namespace ac3mi
