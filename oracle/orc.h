/* oracle/orc.h — TEST INFRASTRUCTURE ONLY.
 *
 * C declarations of the CPU oracle (liborc.so): our own restatement of the
 * reference's AC-3 decode path (liba52: parse.c, bit_allocate.c, imdct.c,
 * downmix.c) and encode path (src/ac3enc/ac3enc.cpp).  Only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg may use it; the
 * product (ac-3-acm-codec_amd/) never links or loads it.
 *
 * Pinning status:
 *   decode  — pinned bit-for-bit against oracle/_ref/liba52_ref.so (the real
 *             liba52 compiled from /root/reference) and the fixtures in
 *             tests/golden/ generated from it.
 *   encode  — pinned byte for byte against oracle/_ref/ac3enc_ref.so (the real
 *             ac3enc.cpp, compiled unmodified behind ref_ac3enc_glue.cpp and the
 *             stand-in headers of winstub/) and the fixture recorded from it,
 *             tests/golden/ac3enc_ref.npz: frames, every stage array, tables,
 *             init decisions (tests/test_oracle_vs_ac3enc.py).
 */
#ifndef ORC_H
#define ORC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- decode (mirrors a52dec-0.7.5-cvs/include/a52.h:56-65) ---- */
typedef struct orc_a52 orc_a52_t;

orc_a52_t *orc_a52_init(void);
float *orc_a52_samples(orc_a52_t *st);
int orc_a52_syncinfo(const uint8_t *buf, int *flags, int *sample_rate, int *bit_rate);
int orc_a52_frame(orc_a52_t *st, const uint8_t *buf, int *flags, float *level, float bias);
void orc_a52_dynrng(orc_a52_t *st, float (*call)(float, void *), void *data);
int orc_a52_block(orc_a52_t *st);
void orc_a52_free(orc_a52_t *st);

/* stage taps: which 0..4 = fbw channel, 5 = lfe, 6 = coupling channel */
void orc_a52_get_exp(orc_a52_t *st, int which, uint8_t *dst256);
void orc_a52_get_bap(orc_a52_t *st, int which, int8_t *dst256);
/* coefficient planes of the last block as the transform stage received them
 * (plane order of a52_samples: LFE first when output), and the block-switch flags */
void orc_a52_get_coefs(orc_a52_t *st, float *dst6x256, uint8_t *blksw5);
int orc_a52_get_lfsr(orc_a52_t *st);
void orc_a52_set_lfsr(orc_a52_t *st, int v);
int orc_a52_get_output(orc_a52_t *st);
void orc_a52_get_layout(orc_a52_t *st, int *out8);
void orc_a52_get_deltbae(orc_a52_t *st, int *out6);
long orc_a52_bitpos(orc_a52_t *st);

/* transform-only entry points (liba52/a52_internal.h:106-120) */
void orc_imdct_512(float *data, float *delay, float bias);
void orc_imdct_256(float *data, float *delay, float bias);
int orc_downmix_init(int input, int flags, float *level, float clev, float slev);
int orc_downmix_coeff(float *coeff, int acmod, int output, float level, float clev, float slev);
void orc_downmix(float *samples, int acmod, int output, float bias, float clev, float slev);
void orc_upmix(float *samples, int acmod, int output);
void orc_imdct_tables(float *window256, float *pre1_256, float *post1_128, float *pre2_128, float *post2_64);

/* transform-only oracle (BASELINE configs 2 and 4), layouts as ac3mi_imdct_batch;
 * state_planes [S][12*256] (liba52 sample buffer incl. overlap planes), state_downmixed [S] */
int orc_xform_batch(const float *coef, const uint8_t *blksw, float *state_planes, int *state_downmixed,
                    float *pcm, int n_streams, int frames, int acmod, int lfeon, int output, float bias,
                    float clev, float slev);

/* float(bias 384) -> s16 interleaved WAVE order (src/AC3ASM.asm, saturating/MMX flavour) */
void orc_convert_s16(const float *planes, int16_t *dst, int flags);

/* whole-stream helper used by bench.py's cpu_baseline: decodes n back-to-back
 * frames of frame_bytes each into planar float (6 blocks x nch x 256 per frame) */
int orc_a52_decode_frames(const uint8_t *frames, int n, int frame_bytes, int flags,
                          float level, float bias, float *pcm_or_null);

/* ---- encode (mirrors src/ac3enc/ac3enc.h:6-7, but re-entrant) ---- */
typedef struct orc_ac3enc orc_ac3enc_t;

orc_ac3enc_t *orc_ac3enc_init(int freq, int bitrate, int channels, int *frame_bytes);
int orc_ac3enc_frame(orc_ac3enc_t *s, uint8_t *dst, const int16_t *samples, const uint8_t *chmap);
void orc_ac3enc_free(orc_ac3enc_t *s);

/* stage taps of the last encoded frame */
void orc_ac3enc_get_mdct(orc_ac3enc_t *s, int32_t *dst /*[6][6][256]*/);
void orc_ac3enc_get_exp(orc_ac3enc_t *s, uint8_t *exponent, uint8_t *encoded_exp /*[6][6][256] each*/);
void orc_ac3enc_get_bap(orc_ac3enc_t *s, uint8_t *bap /*[6][6][256]*/);
void orc_ac3enc_get_misc(orc_ac3enc_t *s, uint8_t *exp_strategy /*[6][6]*/, int8_t *exp_samples /*[6][6]*/,
                         int *csnroffst, int *fsnroffst);
void orc_ac3enc_tables(int16_t *costab64, int16_t *sintab64, int16_t *xcos128, int16_t *xsin128,
                       uint16_t *crc256);
void orc_ac3enc_index_tables(uint8_t *fft_rev128, uint8_t *bndtab51, uint8_t *masktab253);
void orc_ac3enc_get_status(orc_ac3enc_t *s, int *search_failed, int *bytes_written);
void orc_ac3enc_set_last(orc_ac3enc_t *s, const int16_t *last /*[6][256]*/);
void orc_ac3enc_get_last(orc_ac3enc_t *s, int16_t *last /*[6][256]*/);
void orc_ac3enc_spec_tables(int16_t *window256, uint8_t *latab256, uint16_t *hth50x3, uint8_t *baptab64,
                            uint8_t *bndsz50, uint16_t *sdecay4, uint16_t *fdecay4, uint16_t *sgain4,
                            uint16_t *dbknee4, uint16_t *floor8, uint16_t *fgain8, uint16_t *freqs3,
                            uint16_t *bitrate19);
void orc_ac3enc_debug_counts(long *collisions, long *negshift);
void orc_ac3enc_set_marker(int v);      /* test aid: default 128 (ac3enc.cpp:1375-1413) */
void orc_ac3enc_set_spare_curve(int *dst1024);  /* measurement aid: spare bits at every offset, see ac3enc_oracle.c */
void orc_ac3enc_set_extra_curve(int *dst1024);  /* ... and the group ceilings in each count, in sixths of a bit */
void orc_ac3enc_mdct512(int32_t *out256, const int16_t *in512);
int orc_ac3enc_encode_frames(int freq, int bitrate, int channels, const int16_t *pcm, int n,
                             const uint8_t *chmap, uint8_t *out_or_null);

#ifdef __cplusplus
}
#endif
#endif
