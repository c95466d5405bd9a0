/* A plain-C host of ac3mi_truepeak_host and ac3mi_truepeak_read for tests/test_truepeak_cpu.py: built with
 * -fsanitize=address,undefined together with a host-only translation of csrc/truepeak.hip (no GPU parts, no libac3mi.so), so
 * that the rule of truepeak_rule.h - the interpolator, the ordering of maxima, the history hand-over, the read-out - runs under
 * the sanitisers on the CPU.  The PCM is read into a heap block of exactly its size and the state lies in one of exactly
 * ac3mi_truepeak_state_bytes(): a read or write one byte outside either is reported.  The file is metered in two calls when it
 * holds more than one frame (the first frame, then the rest), so the state is carried once.
 *   truepeak_main CHANNELS ROLES FILE CEILING  (ROLES: one digit per channel; FILE: s16le, whole frames of 1536 instants)
 *   ->  "result true_peak true_peak_index true_peak_slot sample_peak sample_peak_slot full_scale samples flags reserved-sum
 *        slot_true_peak x 6  slot_sample_peak x 6", then "state" and the state's bytes in hex */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ac3mi.h"

int main(int argc, char **argv)
{
    if (argc != 5) return 2;
    const int channels = atoi(argv[1]);
    if (channels < 1 || channels > 6 || strlen(argv[2]) != (size_t)channels) return 2;
    uint8_t role[6] = {0, 0, 0, 0, 0, 0};
    for (int c = 0; c < channels; c++) role[c] = (uint8_t)(argv[2][c] - '0');
    const uint32_t ceiling = (uint32_t)strtoul(argv[4], NULL, 10);
    FILE *f = fopen(argv[3], "rb");
    if (!f) return 2;
    if (fseek(f, 0, SEEK_END) != 0) { fclose(f); return 2; }
    const long len = ftell(f);
    const long frame = 1536L * 2 * channels;
    if (len < frame || len % frame != 0 || fseek(f, 0, SEEK_SET) != 0) {    /* not whole frames: refused, not read past */
        fclose(f);
        return 2;
    }
    int16_t *pcm = (int16_t *)malloc((size_t)len);
    const size_t nstate = ac3mi_truepeak_state_bytes();
    uint8_t *state = (uint8_t *)calloc(1, nstate);
    const int whole = pcm && state && fread(pcm, 1, (size_t)len, f) == (size_t)len;
    fclose(f);
    if (!whole) {
        free(pcm);
        free(state);
        return 2;
    }
    const int frames = (int)(len / frame);
    int rc = ac3mi_truepeak_host(channels, role, pcm, 1, state);
    if (rc == AC3MI_OK && frames > 1) rc = ac3mi_truepeak_host(channels, role, pcm + 1536 * channels, frames - 1, state);
    ac3mi_truepeak_result r;
    if (rc == AC3MI_OK) rc = ac3mi_truepeak_read(state, ceiling, &r);
    if (rc != AC3MI_OK) {
        printf("error %d\n", rc);
        free(pcm);
        free(state);
        return 1;
    }
    unsigned reserved = 0;
    for (int i = 0; i < 9; i++) reserved += r.reserved[i];
    printf("result %u %llu %u %u %u %u %llu %u %u", r.true_peak, (unsigned long long)r.true_peak_index, (unsigned)r.true_peak_slot,
           r.sample_peak, (unsigned)r.sample_peak_slot, r.full_scale, (unsigned long long)r.samples, (unsigned)r.flags, reserved);
    for (int c = 0; c < 6; c++) printf(" %u", r.slot_true_peak[c]);
    for (int c = 0; c < 6; c++) printf(" %u", r.slot_sample_peak[c]);
    printf("\nstate ");
    for (size_t i = 0; i < nstate; i++) printf("%02x", state[i]);
    printf("\n");
    free(pcm);
    free(state);
    return 0;
}
