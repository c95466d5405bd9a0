/* A plain-C host of ac3mi_frame_scan for tests/test_frame_scan_cpu.py: built with -fsanitize=address,undefined together with
 * a host-only translation of csrc/scan.hip (no GPU parts, no libac3mi.so), so that the walk and its CRC sums run under the
 * sanitisers on the CPU.  The stream is read into a heap block of exactly its length and the list has exactly max_frames
 * entries: a read or write one byte outside either is reported.
 *   scan_main FILE MODE MAX_FRAMES  ->  "info n_frames consumed skipped rejected flags reserved", then "ref offset bytes sizecod" per frame */
#include <stdio.h>
#include <stdlib.h>
#include "ac3mi.h"

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    long len = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t *buf = (uint8_t *)malloc(len > 0 ? (size_t)len : 1);
    if (!buf || (len > 0 && fread(buf, 1, (size_t)len, f) != (size_t)len)) return 2;
    fclose(f);
    const int mode = atoi(argv[2]), max_frames = atoi(argv[3]);
    ac3mi_frame_ref *refs = (ac3mi_frame_ref *)malloc(sizeof(ac3mi_frame_ref) * (size_t)(max_frames > 0 ? max_frames : 1));
    ac3mi_scan_info info;
    const int rc = ac3mi_frame_scan(buf, (size_t)len, mode, max_frames, refs, &info);
    if (rc != AC3MI_OK) {
        printf("error %d\n", rc);
        return 1;
    }
    printf("info %u %u %u %u %u %u\n", info.n_frames, info.consumed, info.skipped, info.rejected, info.flags, info.reserved);
    for (uint32_t i = 0; i < info.n_frames; i++) printf("ref %u %u %u\n", refs[i].offset, (unsigned)refs[i].bytes, (unsigned)refs[i].sizecod);
    free(refs);
    free(buf);
    return 0;
}
