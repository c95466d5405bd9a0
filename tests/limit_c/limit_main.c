/* A plain-C host of ac3mi_limit_host and ac3mi_limit_read for tests/test_limit_cpu.py: built with -fsanitize=address,undefined
 * together with a host-only translation of csrc/limit.hip (no GPU parts, no libac3mi.so), so that the rule of limit_rule.h -
 * the detector, the quotient, the hold, the release, the smoothing, the delayed application, the read-out - runs under the
 * sanitisers on the CPU.  The PCM and the output lie in heap blocks of exactly their size and the state in one of exactly
 * ac3mi_limit_state_bytes(): a read or write one byte outside any of them is reported.  The file is limited in two calls when
 * it holds more than one frame (the first frame, then the rest), so the state is carried once; then once more in place on a
 * second state, and the two outputs and states are compared with each other and with the expected files.
 *   limit_main CHANNELS ROLES CEILING STEP PCM_FILE WANT_OUT_FILE WANT_STATE_FILE
 *     (ROLES: one digit per channel; files: s16le whole frames of 1536 instants, and the state's bytes)
 *   ->  "result samples reduced max_detect min_gain_q24 flags reserved-sum";  exit 0 = all equal, 3 = a difference */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ac3mi.h"

static void *slurp(const char *path, long *len)
{
    FILE *f = fopen(path, "rb");
    if (!f) return NULL;
    void *p = NULL;
    if (fseek(f, 0, SEEK_END) == 0 && (*len = ftell(f)) > 0 && fseek(f, 0, SEEK_SET) == 0) {
        p = malloc((size_t)*len);
        if (p && fread(p, 1, (size_t)*len, f) != (size_t)*len) {
            free(p);
            p = NULL;
        }
    }
    fclose(f);
    return p;
}

int main(int argc, char **argv)
{
    if (argc != 8) return 2;
    const int channels = atoi(argv[1]);
    if (channels < 1 || channels > 6 || strlen(argv[2]) != (size_t)channels) return 2;
    uint8_t role[6] = {0, 0, 0, 0, 0, 0};
    for (int c = 0; c < channels; c++) role[c] = (uint8_t)(argv[2][c] - '0');
    const uint32_t ceiling = (uint32_t)strtoul(argv[3], NULL, 10), step = (uint32_t)strtoul(argv[4], NULL, 10);
    const size_t nstate = ac3mi_limit_state_bytes();
    const long frame = 1536L * 2 * channels;
    long len = 0, want_len = 0, state_len = 0;
    int16_t *pcm = (int16_t *)slurp(argv[5], &len);
    int16_t *want = (int16_t *)slurp(argv[6], &want_len);
    uint8_t *want_state = (uint8_t *)slurp(argv[7], &state_len);
    int rc = 2;
    int16_t *out = NULL, *inplace = NULL;
    uint8_t *state = NULL, *state2 = NULL;
    /* not whole frames, or files that do not belong together: refused, not read past */
    if (pcm && want && want_state && len >= frame && len % frame == 0 && want_len == len && (size_t)state_len == nstate) {
        out = (int16_t *)malloc((size_t)len);
        inplace = (int16_t *)malloc((size_t)len);
        state = (uint8_t *)calloc(1, nstate);
        state2 = (uint8_t *)calloc(1, nstate);
    }
    if (out && inplace && state && state2) {
        const int frames = (int)(len / frame);
        memcpy(inplace, pcm, (size_t)len);
        rc = ac3mi_limit_host(channels, role, ceiling, step, pcm, out, 1, state);
        if (rc == AC3MI_OK && frames > 1)
            rc = ac3mi_limit_host(channels, role, ceiling, step, pcm + 1536 * channels, out + 1536 * channels, frames - 1, state);
        if (rc == AC3MI_OK) rc = ac3mi_limit_host(channels, role, ceiling, step, inplace, inplace, frames, state2);
        /* a partial overlap is refused and touches nothing */
        if (rc == AC3MI_OK && frames > 1 &&
            ac3mi_limit_host(channels, role, ceiling, step, inplace, inplace + 768 * channels, frames - 1, state2) != AC3MI_ERR_ARG)
            rc = 3;
        ac3mi_limit_result r;
        if (rc == AC3MI_OK) rc = ac3mi_limit_read(state, &r);
        if (rc == AC3MI_OK) {
            unsigned reserved = 0;
            for (int i = 0; i < 7; i++) reserved += r.reserved[i];
            printf("result %llu %llu %u %u %u %u\n", (unsigned long long)r.samples, (unsigned long long)r.reduced, r.max_detect, r.min_gain_q24,
                   (unsigned)r.flags, reserved);
            if (memcmp(out, want, (size_t)len) != 0 || memcmp(inplace, want, (size_t)len) != 0 || memcmp(state, want_state, nstate) != 0 ||
                memcmp(state2, want_state, nstate) != 0)
                rc = 3;
        } else if (rc != 3) {
            printf("error %d\n", rc);
            rc = 1;
        }
    }
    free(pcm);
    free(want);
    free(want_state);
    free(out);
    free(inplace);
    free(state);
    free(state2);
    return rc;
}
