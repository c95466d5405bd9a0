/* oracle/ref_ac3enc_glue.cpp — TEST INFRASTRUCTURE ONLY.
 *
 * Our own accessor around the reference's UNMODIFIED encoder: ac3enc.cpp is pulled in by path at
 * compile time (-I$(ENCREF), the pattern of ref_ac3tab_glue.cpp) behind the two stand-in headers of
 * oracle/winstub/ (32-bit `long`, counting _ASSERT) and -D_AMD64_ (its portable byte swap), into
 * oracle/_ref/ac3enc_ref.so.  It hands out the two entry points, the file-static stage arrays of the
 * last frame, the search result, the tables that the encoder fills at run time, and the number of
 * reference assertions that did not hold.
 *
 * The reference keeps ONE static context and AC3_encode_init does not clear all of it.  A fresh
 * instance per stream is therefore a PRIVATELY COPIED LIBRARY per stream: the caller
 * (tests/_harness.RefEncoder) copies ac3enc_ref.so to a temporary file and loads that copy, so every
 * stream starts from zero-initialised statics; only the re-initialisation cases encode two streams
 * in one copy on purpose.
 */
#include <string.h>
#include <type_traits>
#include <ac3enc.cpp>
#undef long

extern "C" {

int refenc_init(int freq, int bitrate, int channels) { return AC3_encode_init(freq, bitrate, channels); }

/* dst must hold AC3_MAX_CODED_FRAME_SIZE bytes and slack: the bit writer does not check its end */
int refenc_frame(unsigned char *dst, short *samples, unsigned char *chmap) { return AC3_encode_frame(dst, samples, chmap); }

const void *refenc_array(const char *name, int *count, int *elem_bytes)
{
#define ELEM(t) sizeof(std::remove_all_extents<decltype(t)>::type)
#define ARR(t) if (!strcmp(name, #t)) { *count = (int)(sizeof(t) / ELEM(t)); *elem_bytes = (int)ELEM(t); return (const void *)(t); }
    ARR(mdct_coef) ARR(exponent) ARR(exp_strategy) ARR(encoded_exp) ARR(bap) ARR(exp_samples)
    ARR(costab) ARR(sintab) ARR(xcos1) ARR(xsin1) ARR(fft_rev) ARR(crc_table) ARR(bndtab) ARR(masktab)
#undef ARR
#undef ELEM
    *count = 0;
    *elem_bytes = 0;
    return 0;
}

/* out[0] csnroffst, out[1..6] fsnroffst per channel, out[7..12] fgaincod per channel */
void refenc_snr(int *out13)
{
    out13[0] = ac3enc_state.csnroffst;
    for (int ch = 0; ch < AC3_MAX_CHANNELS; ch++) {
        out13[1 + ch] = ac3enc_state.fsnroffst[ch];
        out13[7 + ch] = ac3enc_state.fgaincod[ch];
    }
}

/* how many of the reference's _ASSERT conditions did not hold so far; sites32: { source line, trips } of up to 16 sites */
int refenc_assert_trips(int *sites32)
{
    if (sites32) memcpy(sites32, winstub_assert_site, sizeof winstub_assert_site);
    return winstub_assert_trips;
}

}
