/* csrc/sync_rule.h on the host, for tests/test_header_rule_cpu.py: built without HIP, with -fsanitize=address,undefined, and
 * run on its own (never loaded into Python).  For each of the sync words 0x0b77, 0x0b76, 0x770b, 0x0000 and every (byte 4,
 * byte 5), in that order, one line
 *     size size_le fscod halfrate
 * size: the byte form (sync_header_ok, sync_frame_bytes); size_le: the masked-dword form the frame scan uses (scan_rule.h's
 * scan_header_size on two little-endian dwords), bytes 2-3 and 6-7 - which neither form looks at - drawn from SEED.
 * Then one line per acmod 0..7: sync_lfeon_pos.
 *   header_rule SEED */
#include <stdio.h>
#include <stdlib.h>
#include "sync_rule.h"
#include "scan_rule.h"

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    uint32_t lcg = (uint32_t)strtoul(argv[1], nullptr, 10);
    static const uint32_t syncs[4] = {0x0b77u, 0x0b76u, 0x770bu, 0x0000u};
    for (uint32_t sync : syncs)
        for (uint32_t b4 = 0; b4 < 256; b4++)
            for (uint32_t b5 = 0; b5 < 256; b5++) {
                lcg = lcg * 1664525u + 1013904223u;
                const uint32_t w0 = (sync >> 8) | (sync & 0xffu) << 8 | (lcg & 0xffff0000u);
                const uint32_t w1 = b4 | b5 << 8 | (lcg << 16);
                const uint32_t size = ac3mi::sync_header_ok(sync, b4, b5) ? ac3mi::sync_frame_bytes(b4) : 0u;
                printf("%u %u %u %d\n", size, ac3mi::scan_header_size(w0, w1), b4 >> 6, ac3mi::sync_halfrate((int)(b5 >> 3)));
            }
    for (int acmod = 0; acmod < 8; acmod++) printf("%d\n", ac3mi::sync_lfeon_pos(acmod));
    return 0;
}
