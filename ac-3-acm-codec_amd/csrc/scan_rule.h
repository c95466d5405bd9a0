// scan_rule.h — the framing rule of ac3mi_frame_scan / ac3mi_frame_scan_batch (include/ac3mi.h), the part that needs no GPU:
// the header test and the frame's size on a candidate's first two dwords (sync_rule.h's, which the host walk below and
// frame_scan_kernel in scan.hip both call), and the host walk itself, stream_convert_ac3's resync rule (run_decode in
// stream.hip) with the two CRC sums of crc.hip in plain C.
// Plain C++: compiles without HIP (a host-only build of scan.hip for the sanitiser program of tests/frame_scan_c).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/ac3mi.h"

#include "sync_rule.h"

namespace ac3mi {

// w0 = bytes 0-3 of a candidate, w1 = bytes 4-7, each little-endian: the frame's size in bytes; 0: the test refuses the header
__host__ __device__ inline uint32_t scan_header_size(uint32_t w0, uint32_t w1)
{
    return sync_header_ok_le(w0, w1) ? sync_frame_bytes(w1 & 0xffu) : 0;
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
