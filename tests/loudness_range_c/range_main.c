/* A plain-C host of ac3mi_loudness_range_read for tests/test_loudness_range_cpu.py: built with -fsanitize=address,undefined
 * together with a host-only translation of csrc/loudness.hip (no GPU parts, no libac3mi.so), so that the read-out rule of
 * loudness_rule.h - the relative gate, the bins that count, the two ranks and their bins - runs under the sanitisers on the
 * CPU.  Each state is read into a heap block of exactly ac3mi_loudness_range_state_bytes(): a read one byte outside it is
 * reported.
 *   range_main < STATES  ->  per state "result max_short_energy-bits lra-bits low_lkfs-bits high_lkfs-bits max_short_lkfs-bits
 *                            blocks blocks_abs blocks_rel lra_tenths low_bin high_bin flags reserved-sum"
 * (the floats as the hexadecimal of their bits: the output is compared exactly).  Input that is not whole states: exit 2. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ac3mi.h"

static unsigned bits32(float v)
{
    unsigned u;
    memcpy(&u, &v, sizeof u);
    return u;
}

int main(void)
{
    const size_t len = ac3mi_loudness_range_state_bytes();
    for (;;) {
        uint8_t *buf = (uint8_t *)malloc(len);
        if (!buf) return 2;
        const size_t got = fread(buf, 1, len, stdin);
        if (got != len) {
            free(buf);
            return got == 0 && feof(stdin) ? 0 : 2;
        }
        ac3mi_loudness_range_result r;
        const int rc = ac3mi_loudness_range_read(buf, &r);
        free(buf);
        if (rc != AC3MI_OK) {
            printf("error %d\n", rc);
            return 1;
        }
        unsigned long long e;
        memcpy(&e, &r.max_short_energy, sizeof e);
        unsigned reserved = 0;
        for (int i = 0; i < 5; i++) reserved += r.reserved[i];
        printf("result %016llx %08x %08x %08x %08x %u %u %u %u %u %u %u %u\n", e, bits32(r.lra), bits32(r.low_lkfs), bits32(r.high_lkfs),
               bits32(r.max_short_lkfs), r.blocks, r.blocks_abs, r.blocks_rel, (unsigned)r.lra_tenths, (unsigned)r.low_bin,
               (unsigned)r.high_bin, (unsigned)r.flags, reserved);
    }
}
