/* A plain-C host of ac3mi_loudness_read for tests/test_loudness_cpu.py: built with -fsanitize=address,undefined together with
 * a host-only translation of csrc/loudness.hip (no GPU parts, no libac3mi.so), so that the read-out rule of loudness_rule.h -
 * the bin walk, the relative gate, the bin the gate cuts, the dialnorm decision - runs under the sanitisers on the CPU.  The
 * state is read into a heap block of exactly ac3mi_loudness_state_bytes(): a read one byte outside it is reported.
 *   loudness_main FILE  ->  "result mean_energy max_block_energy lkfs blocks blocks_abs blocks_rel dialnorm flags reserved-sum" */
#include <stdio.h>
#include <stdlib.h>
#include "ac3mi.h"

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const size_t len = ac3mi_loudness_state_bytes();
    uint8_t *buf = (uint8_t *)malloc(len);
    const int whole = buf && fread(buf, 1, len, f) == len && fgetc(f) == EOF;
    fclose(f);
    if (!whole) {
        free(buf);
        return 2;
    }
    ac3mi_loudness_result r;
    const int rc = ac3mi_loudness_read(buf, &r);
    if (rc != AC3MI_OK) {
        printf("error %d\n", rc);
        return 1;
    }
    unsigned reserved = 0;
    for (int i = 0; i < 6; i++) reserved += r.reserved[i];
    printf("result %.17g %.17g %.9g %u %u %u %u %u %u\n", r.mean_energy, r.max_block_energy, (double)r.lkfs, r.blocks, r.blocks_abs,
           r.blocks_rel, (unsigned)r.dialnorm, (unsigned)r.flags, reserved);
    free(buf);
    return 0;
}
