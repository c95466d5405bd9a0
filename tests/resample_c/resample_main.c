/* A plain-C host of ac3mi_resample_host, _plan, _ratio and _tables for tests/test_resample_cpu.py: built with
 * -fsanitize=address,undefined together with a host-only translation of csrc/resample.hip (no GPU parts, no libac3mi.so), so
 * that the rule of resample_rule.h - the table's design and split, the plan, an output instant, the elastic buffer - runs under
 * the sanitisers on the CPU.  The PCM, every call's output and the table lie in heap blocks of exactly their size and the state
 * in one of exactly ac3mi_resample_state_bytes(): a read or write one byte outside any of them is reported.  The file is
 * converted in two calls when it holds more than one frame (the first frame, then the rest), each with its planned out_frames,
 * then once more in one call on a second state; the outputs and states are compared with each other and with the expected
 * files.  A call with a wrong out_frames must give status 1, zeros, and leave the state alone.
 *   resample_main IN_RATE OUT_RATE CHANNELS PCM_FILE WANT_OUT_FILE WANT_STATE_FILE
 *     (files: s16le whole frames of 1536 instants - WANT_OUT_FILE may be empty - and the state's bytes)
 *   ->  "result out_frames pending table-sum";  exit 0 = all equal, 3 = a difference */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ac3mi.h"

static void *slurp(const char *path, long *len)
{
    FILE *f = fopen(path, "rb");
    if (!f) return NULL;
    void *p = NULL;
    if (fseek(f, 0, SEEK_END) == 0 && (*len = ftell(f)) >= 0 && fseek(f, 0, SEEK_SET) == 0) {
        p = malloc(*len > 0 ? (size_t)*len : 1);
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
    if (argc != 7) return 2;
    ac3mi_resample_desc desc;
    desc.in_rate = atoi(argv[1]);
    desc.out_rate = atoi(argv[2]);
    desc.channels = atoi(argv[3]);
    int L = 0, M = 0, taps = 0;
    if (ac3mi_resample_ratio(desc.in_rate, desc.out_rate, &L, &M, &taps) != AC3MI_OK || desc.channels < 1 || desc.channels > 6) return 2;
    const size_t nstate = ac3mi_resample_state_bytes();
    const long frame = 1536L * 2 * desc.channels;
    long len = 0, want_len = 0, state_len = 0;
    int16_t *pcm = (int16_t *)slurp(argv[4], &len);
    int16_t *want = (int16_t *)slurp(argv[5], &want_len);
    uint8_t *want_state = (uint8_t *)slurp(argv[6], &state_len);
    int rc = 2;
    /* not whole frames, or files that do not belong together: refused, not read past */
    if (pcm && want && want_state && len >= frame && len % frame == 0 && want_len % frame == 0 && (size_t)state_len == nstate) {
        const int frames = (int)(len / frame);
        int of1 = 0, of2 = 0, all = 0, left = 0, left_all = 0;
        rc = ac3mi_resample_plan(desc.in_rate, desc.out_rate, 0, 0, 1, &of1, &left);
        if (rc == AC3MI_OK && frames > 1) rc = ac3mi_resample_plan(desc.in_rate, desc.out_rate, 1536, (uint64_t)of1, frames - 1, &of2, &left);
        if (rc == AC3MI_OK) rc = ac3mi_resample_plan(desc.in_rate, desc.out_rate, 0, 0, frames, &all, &left_all);
        if (rc == AC3MI_OK && (of1 + of2 != all || left != left_all || (long)all * frame != want_len)) rc = 3;
        int32_t *coef = (int32_t *)malloc(sizeof(int32_t) * (size_t)L * (size_t)taps);
        int16_t *a = of1 ? (int16_t *)malloc((size_t)of1 * (size_t)frame) : NULL, *b = of2 ? (int16_t *)malloc((size_t)of2 * (size_t)frame) : NULL;
        /* what the stream would have to take next, and one frame more: a count that is not its own */
        int wrong = 0;
        if (rc == AC3MI_OK) rc = ac3mi_resample_plan(desc.in_rate, desc.out_rate, 1536u * (uint64_t)frames, (uint64_t)all, frames, &wrong, NULL);
        wrong += 1;
        int16_t *whole = all ? (int16_t *)malloc((size_t)all * (size_t)frame) : NULL, *bad = (int16_t *)malloc((size_t)wrong * (size_t)frame);
        uint8_t *state = (uint8_t *)calloc(1, nstate), *state2 = (uint8_t *)calloc(1, nstate), *kept = (uint8_t *)malloc(nstate);
        if (rc == AC3MI_OK && coef && (a || !of1) && (b || !of2) && (whole || !all) && bad && state && state2 && kept) {
            uint32_t st1 = 9, st2 = 0, st3 = 9, st4 = 9;
            long long sum = 0;
            rc = ac3mi_resample_tables(desc.in_rate, desc.out_rate, coef);
            for (long i = 0; rc == AC3MI_OK && i < (long)L * taps; i++) sum += coef[i];
            if (rc == AC3MI_OK) rc = ac3mi_resample_host(&desc, pcm, 1, a, of1, state, &st1);
            if (rc == AC3MI_OK && frames > 1) {
                st2 = 9;
                rc = ac3mi_resample_host(&desc, pcm + 1536 * desc.channels, frames - 1, b, of2, state, &st2);
            }
            if (rc == AC3MI_OK) rc = ac3mi_resample_host(&desc, pcm, frames, whole, all, state2, &st3);
            /* a frame too many: refused for the stream, which stays as it is */
            memcpy(kept, state2, nstate);
            memset(bad, 0x5a, (size_t)wrong * (size_t)frame);
            if (rc == AC3MI_OK) rc = ac3mi_resample_host(&desc, pcm, frames, bad, wrong, state2, &st4);
            if (rc == AC3MI_OK) {
                printf("result %d %d %lld\n", all, left_all, sum);
                if (st1 || st2 || st3 || st4 != AC3MI_RESAMPLE_FRAMES || memcmp(kept, state2, nstate) != 0) rc = 3;
                for (long i = 0; i < (long)wrong * (frame / 2); i++)
                    if (bad[i] != 0) rc = 3;
                if ((of1 && memcmp(a, want, (size_t)of1 * (size_t)frame) != 0) ||
                    (of2 && memcmp(b, (const char *)want + (size_t)of1 * (size_t)frame, (size_t)of2 * (size_t)frame) != 0) ||
                    (all && memcmp(whole, want, (size_t)all * (size_t)frame) != 0) || memcmp(state, want_state, nstate) != 0 ||
                    memcmp(state2, want_state, nstate) != 0)
                    rc = 3;
            } else {
                printf("error %d\n", rc);
                rc = 1;
            }
        } else if (rc == AC3MI_OK) {
            rc = 1;
        }
        free(coef);
        free(a);
        free(b);
        free(whole);
        free(bad);
        free(state);
        free(state2);
        free(kept);
    }
    free(pcm);
    free(want);
    free(want_state);
    return rc;
}
