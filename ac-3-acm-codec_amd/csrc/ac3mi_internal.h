// ac3mi_internal.h — host-side declarations shared by the translation units of libac3mi.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <array>
#include <string>
#include <utility>
#include <vector>
#include "../../include/ac3mi.h"
#include "launch_rule.h"

namespace ac3mi {

// decoder front-end tables (device copy)
struct DecTables {
    int8_t la_neg[256];
    uint16_t hth[3][50];
    int8_t width[64];
    uint8_t band_end[30];
    uint8_t band_of_bin[256];   // band of a bin (bins 0..27 are their own band)
    float qlev[48];     // [0,3) 3-level  [3,8) 5-level  [8,16) 7-level  [16,27) 11-level  [27,43) 15-level
    // dequantised value of member m of a code: 3-level [code*3+m] at 0 (32 codes), 5-level at 96 (128 codes),
    // 11-level [code*2+m] at 480 (128 codes), 7-level [code] at 736, 15-level [code] at 744; reserved codes give 0
    float qtab[760];
    uint32_t desc[128];     // per row byte of the bap rows: see mant_desc (decode_common.h)
};

// encoder tables (device copy): ENC/ac3tab.h + the runtime tables of AC3_encode_init
struct EncTables {
    int16_t win[256];           // ac3_window, Q15
    int16_t cos[64], sin[64];   // costab / sintab (fft_init(7))
    int16_t xcos[128], xsin[128];
    uint8_t bitrev[128];
    uint8_t latab[256];
    uint16_t hth[50][3];
    uint8_t baptab[64];
    uint8_t band_of_bin[256];   // masktab
    uint8_t band_start[51];     // bndtab (entry 50 = 0 as in ac3_common_init)
    uint8_t band_size[50];      // bndsz
    uint16_t crc_tab[256];
    int16_t xcos2[64], xsin2[64];   // the short transform pair's pre/post-rotation (256-point MDCT: xcos1/xsin1 at N = 256)
};

// what AC3_encode_init derives from (freq, bitrate, channels): ENC/ac3enc.cpp:1019-1110
struct EncConfig {
    int nch, nfbw, lfe, acmod, fscod, halfrate, bsid, frmsizecod, frame_words;
};

// Device-resident constant tables, built on the host in double precision.
struct DeviceTables {
    float2 *tw_long;    // [8][16]  merged lane twiddles, long block
    float2 *tw_short;   // [8][16]  merged lane twiddles, short block
    float *window;      // [256]    KBD alpha=5 window (L52/imdct.c:364-372)
    DecTables *dec;     // bit-allocation / dequantiser tables
    uint16_t *lfsr_seq; // [65535] dither LFSR states in cycle order from state 1 (L52/parse.c:310-319)
    uint16_t *lfsr_idx; // [65536] inverse: position of a state in the cycle
    EncTables *enc;
};

struct MixPlan {
    int n_in, n_out, nfchans, in_lfe;
    // mix[o][c]: weight (-1, 0, +1) of input plane c in output plane o
    int8_t mix[6][6];
    // Surround planes that liba52 mixes at level slev into MONO / STEREO / 3F (bit c = input plane c), 0 elsewhere: when a
    // frame's slev is 0 liba52 neither transforms nor mixes them (L52/parse.c:900-913, downmix.c:494-583), which is not a
    // linear mix at level 0 as far as their overlap tails go - see XformLaunch::mix_pending.
    uint8_t surr_mask;
    // ... and the OUTPUT planes that then come out without the bias when the block takes the per-channel path: for 2/1 and
    // 2/2 to STEREO and 3/1 and 3/2 to 3F a52_downmix returns at `if (slev == 0) break;` (downmix.c:530-583) before the
    // mixer that would have added it, and a52_downmix_coeff had told a52_block not to add it in those channels' transforms
    uint8_t nobias_mask;
};

// every coded plane is an output plane, routed to itself: no mixing
inline bool mix_plan_identity(const MixPlan &plan)
{
    if (plan.n_in != plan.n_out) return false;
    for (int o = 0; o < plan.n_out; o++)
        for (int c = 0; c < plan.n_in; c++)
            if (plan.mix[o][c] != (o == c ? 1 : 0)) return false;
    return true;
}

struct XformLaunch {
    const float *coef;
    const uint8_t *blksw;
    float *delay;
    float *pcm;
    int n_streams, frames;
    int blocks = 0;         // 0: frames x 6 blocks per stream; else exactly this many blocks (a52_imdct_512/256 hooks: 1)
    float bias;
    MixPlan plan;
    const int32_t *slot;    // optional per-stream state slot indices (device), see ac3mi_set_state_slots
    int delay_stride;
    // s16 output instead of float planes: [n_streams][frames][6][256][n_out] interleaved in WAVE channel order, what the
    // reference's MapTab converters make of a52_samples() at bias 384 (src/AC3ASM.asm; s16_channel_map).  pcm is unused then.
    int16_t *pcm16 = nullptr;
    int s16_flags = 0;      // liba52 output flags of the planes (selects the channel order)
    // liba52's overlap bookkeeping around frames whose surround mix level is 0 (ac3mi_set_mix_state): per frame "slev is 0"
    // from the decode front end, per output chain the surround planes' share of the overlap tail that is held back
    // ([streams or slots][n_out][128], laid out like `delay`) and its flags ([streams or slots][6]: bit 0 liba52's
    // `downmixed`, bit 1 share pending).  All three null: a plain linear mix.
    const uint8_t *zs = nullptr;
    float *mix_pending = nullptr;
    int32_t *mix_flags = nullptr;
};

// a52_downmix()/a52_downmix_init() semantics as a plane-mixing matrix; returns <0 if
// `output` is not a configuration liba52 grants for `acmod`.
int build_mix_plan(int acmod, int lfeon, int output, MixPlan *plan);

hipError_t launch_xform(const DeviceTables &tab, const XformLaunch &L, hipStream_t stream);

// what the host needs of the split front end's block descriptor (BlkDesc, mant2.h, asserts both): its size, and the byte
// offset of src_snr, the word a transcode's encoder reads as its search hint
constexpr int BLKDESC_BYTES = 80, BLKDESC_SRC_SNR = 72;

struct DecodeLaunch {
    const uint8_t *frames;
    int frame_bytes, frame_stride, n_streams, frames_per_stream;
    int req_flags, acmod, lfeon, dynrng_on;
    float level;
    float *coef;            // [S][F][6][n_in][256]
    uint8_t *blksw;         // [S][F][6][nfchans]
    uint32_t *status;       // [S][F]
    uint16_t *lfsr;         // [S]
    uint8_t *tap_exp;
    int8_t *tap_bap;
    uint8_t *zs = nullptr;              // optional [S][F]: 1 = the frame's surround channels are mixed at level 0 (see XformLaunch)
    float *dyn_out = nullptr;           // [S][F][6][2] range factors of the stream's dynamic-range words (NaN: none)
    const float *dyn_in = nullptr;      // [S][F][6][2] replacements (NaN: keep)
    const int32_t *slot;
    // the front end and its kernels (launch_rule.h): the launchers launch choice.launch in order
    DecChoice choice;
    // frame-parallel (choice.fp): workspaces
    uint32_t *frame_draws;  // [S][F] workspace
    uint16_t *frame_lfsr;   // [S][F] workspace
    // split front end (choice.split: parse kernel + one wavefront per audio block): workspaces, all or none
    void *ws_desc = nullptr;        // [S][F][6] BlkDesc (BLKDESC_BYTES)
    uint8_t *ws_rows = nullptr;     // [S][F][6][7][512]
    float *ws_cplco = nullptr;      // [S][F][6][90]
    uint32_t *ws_fpos = nullptr;    // [S][F]
    // split front end, one-frame streams, identity routing: mantissas + transform in one kernel (decode_mx.hip) - no
    // coefficient planes in HBM (coef unused), the caller does not launch the transform
    const XformLaunch *fuse = nullptr;
    // ac3mi_set_decode_crc 1 / 2: the CRC kernel's verdict byte per frame, [S][F] (crc.hip); null: the frames are not checked
    const uint8_t *crc = nullptr;
    // ac3mi_set_encode_drc_source 1 (transcode): [S][F][6] the raw dynamic-range fields of every block the front end reads - bit 8
    // dynrnge, bits 0-7 dynrng, bit 24 dynrng2e, bits 16-23 dynrng2 (acmod 0) - for enc_dynrng_source_kernel.  Non-null: the SRC
    // instantiations of the front ends run (generic shape only); a block that is not reached leaves its word unwritten
    uint32_t *src_dyn = nullptr;
    const LaunchLog *log = nullptr;     // ac3mi_debug_launch_log: the launchers append what they launch (launch_rule.h); null: no tap
};
hipError_t launch_decode(const DeviceTables &tab, const DecodeLaunch &L, hipStream_t stream);
// decode_wg.hip: one workgroup per stream; X == nullptr: coefficient planes (+ taps) to HBM as launch_decode does;
// else the transform is fused in (identity routing only: returns hipErrorInvalidValue for a mixing plan)
hipError_t launch_decode_wg(const DeviceTables &tab, const DecodeLaunch &L, const XformLaunch *X, int grid_cap, hipStream_t stream);
void build_dec_tables(DecTables *t, uint16_t *lfsr_seq /*[65535]*/, uint16_t *lfsr_idx /*[65536]*/);

// crc.hip: one wavefront per frame sums the frame's two CRC regions; verdict[i]: bit 0 crc1's region fails, bit 1 crc2's,
// bit 6 (with `conceal`, when either fails) the front end is to refuse the frame, bit 7 not summed - the header test on bytes
// 0-5 failed, the frame is longer than frame_bytes, or (acmod >= 0) its acmod / lfeon are not these
struct CrcLaunch {
    const uint8_t *frames;
    uint8_t *verdict;
    size_t n_frames;
    int frame_stride, frame_bytes;
    int acmod = -1, lfeon = 0;
    bool conceal = false;
};
hipError_t launch_crc(const CrcLaunch &L, hipStream_t stream);

// ac3mi_set_encode_coupling 1: what the coupling kernel leaves per frame for the search and the packer
struct CplWs {
    uint32_t *word;             // [F] bit 0 cplinu, bits 8 + 2 ch .. 9 + 2 ch: mstrcplco of channel ch
    uint8_t *co;                // [F][5][16] cplcoexp << 4 | cplcomant per channel and band
    int32_t *mdct;              // [F][6][256] the coupling rows (bins outside [cplstrtmant, cplendmant): 0)
    int8_t *shift;              // [F][8] their exp_samples
    uint8_t *eexp;              // [F][6][256] encoded exponents; bin cplstrtmant - 1 holds 2 cplabsexp
    int16_t *emask;             // [F][6][50] masking curves minus the floor
    uint8_t *strat;             // [F][8] cplexpstr
    int32_t *ebits;             // [F] bits of cplabsexp and the exponent groups
    // 2/0 with rematrixing on (else null): the rows and exponent stage of enc_mdct_kernel without rematrixing, from which a
    // coupled frame's rematrixing is decided again over liba52's cplinu-1 band set
    int32_t *prow;              // [F][6][2][256]
    int8_t *pshift;             // [F][6][2]
    uint8_t *peexp;             // [F][6][2][256]
    int16_t *pemask;            // [F][6][2][50]
    uint8_t *pstrat;            // [F][6][2]
    int32_t *pebits;            // [F][2]
    // (2/0+LFE: every p* array has three rows per block instead of two, the LFE's last - [F][6][3][256] etc.)
};
constexpr int CPL_FRAME_BYTES = 16 + 80 + 6 * 256 * 4 + 8 + 6 * 256 + 6 * 50 * 2 + 8 + 8;
// the p* arrays of one frame with `nrow` rows a block (2: 2/0, 3: 2/0+LFE), each array's frames rounded up to 16 bytes
constexpr int cpl_remat_frame_bytes(int nrow)
{
    return 6 * nrow * 256 * 4 + ((6 * nrow + 15) & ~15) + 6 * nrow * 256 + 6 * nrow * 50 * 2 + ((6 * nrow + 15) & ~15) +
           ((4 * nrow + 15) & ~15);
}
constexpr int CPL_REMAT_FRAME_BYTES = cpl_remat_frame_bytes(2);
static_assert(CPL_REMAT_FRAME_BYTES == 6 * 2 * 256 * 4 + 16 + 6 * 2 * 256 + 6 * 2 * 50 * 2 + 16 + 16, "2/0 layout");

// The sanitising rule (include/ac3mi.h, ac3mi_bsi_info): what a raw bsi_word becomes before the packers code it - dialnorm 0
// (reserved) 31, cmixlev 3 and surmixlev 3 the levels liba52's tables give the reserved code (1), dsurmod 3 0; bsmod,
// copyrightb and origbs pass.  The BSI reader (bsi.hip) and the encoder's per-frame words (encode.hip) both go through it.
__host__ __device__ constexpr uint32_t bsi_sanitise(uint32_t w)
{
    w &= 0xffffu;
    if ((w & 31u) == 0) w |= 31u;
    if ((w & 0x300u) == 0x300u) w ^= 0x200u;
    if ((w & 0xc00u) == 0xc00u) w ^= 0x800u;
    if ((w & 0x3000u) == 0x3000u) w ^= 0x3000u;
    return w;
}
static_assert(bsi_sanitise(BSI_DEFAULT) == BSI_DEFAULT && bsi_sanitise(bsi_word(0, 5, 3, 3, 3, 1, 0)) == bsi_word(31, 5, 1, 1, 0, 1, 0), "rule");

// bsi.hip: one lane per frame reads bytes 0-5 and the BSI.  `info` (ac3mi_bsi_read_batch): the record of every frame.
// `words` (ac3mi_set_encode_metadata_source 1, ahead of a transcode's encoder): per frame the bsi_word the new frame codes -
// the source's dialnorm, bsmod, copyrightb, origbs, and cmixlev / surmixlev / dsurmod where the source sent the field and
// `coded_acmod` sends it, else ctx_word's; ctx_word whole for a frame the decoder refuses (header test, frame_bytes, another
// acmod / lfeon than the call's, or bit 6 of its `crc` verdict byte - crc may be null).  Exactly one of info / words is set.
struct BsiLaunch {
    const uint8_t *frames;
    size_t n_frames;
    int frame_stride, frame_bytes;
    ac3mi_bsi_info *info = nullptr;
    uint32_t *words = nullptr;
    const uint8_t *crc = nullptr;
    int acmod = 0, lfeon = 0, coded_acmod = 0;
    uint32_t ctx_word = BSI_DEFAULT;
};
hipError_t launch_bsi(const BsiLaunch &L, hipStream_t stream);

// bsi.hip, enc_dynrng_source_kernel (ac3mi_set_encode_drc_source 1, after a transcode's front end and ahead of its encoder): one
// lane per frame resolves the source's words into the arrays of ac3mi_set_encode_dynrng_frames - `codes` [n][6][2] the code in
// force in every block (0 at the frame's start, a word holds to its end), `compr` [n][2] - from the front end's raw words
// (DecodeLaunch::src_dyn), the frame's own BSI and its status word: a frame with bit 8 or any of bits 0-5 set carries nothing.
// prog: -1 both programmes of a dual-mono source (coded as dual mono), else the one programme (0, 1) that becomes programme 0
struct DynSrcLaunch {
    const uint8_t *frames;
    size_t n_frames;
    int frame_stride, frame_bytes;
    const uint32_t *src_dyn;
    const uint32_t *status;
    uint8_t *codes;
    uint16_t *compr;
    int prog = 0;
};
hipError_t launch_dynrng_source(const DynSrcLaunch &L, hipStream_t stream);
void bsi_read_host(const uint8_t *buf, int len, ac3mi_bsi_info *out);

// scan.hip: frames found in byte streams (ac3mi_frame_scan_batch).  One wavefront per stream walks bytes [0, len[s]) of
// bytes + s * stride by the rule of include/ac3mi.h (mode 1: a candidate counts only if both CRC regions sum to 0) and
// lists up to max_frames frames in refs[s][max_frames] and the walk's end in info[s].  bytes and stride: multiples of 16,
// stride < 2^32; entries of refs at or behind n_frames are not written
struct ScanLaunch {
    const uint8_t *bytes;
    uint64_t stride;
    const uint32_t *len;
    size_t n_streams;
    int mode, max_frames;
    ac3mi_frame_ref *refs;
    ac3mi_scan_info *info;
};
hipError_t launch_frame_scan(const ScanLaunch &L, hipStream_t stream);
// ... and laid out for the batched calls (ac3mi_frame_gather_batch): one wavefront per slot copies frame first_frame + f of
// stream s to frames + (s * frames_per_stream + f) * frame_stride and zeroes the rest of the slot; a slot without a frame, or
// whose frame is longer than frame_bytes, is all zeros.  bytes, stride, frames, frame_stride: multiples of 4
struct GatherLaunch {
    const uint8_t *bytes;
    uint64_t stride;
    size_t n_streams;
    const ac3mi_frame_ref *refs;
    const ac3mi_scan_info *info;
    int max_frames, first_frame, frames_per_stream;
    uint8_t *frames;
    int frame_stride, frame_bytes;
};
hipError_t launch_frame_gather(const GatherLaunch &L, hipStream_t stream);

// loudness.hip: the BS.1770 meter (ac3mi_loudness_*; the rule is include/ac3mi.h's, its decisions loudness_rule.h's).  tab:
// LOUD_TAB_DOUBLES doubles on the device, E_0 .. E_900 then the 30 dialnorm thresholds (loud_fill_tab writes them on the host)
constexpr int LOUD_TAB_DOUBLES = 901 + 30;
void loud_fill_tab(double *h_tab);
struct LoudnessLaunch {
    const int16_t *pcm;             // [S][F][1536][channels]
    int sample_rate, channels;
    uint8_t role[6];
    int n_streams, frames_per_stream;
    void *state;                    // [S] LoudState
    const double *tab;
    void *range_state = nullptr;    // [S] RangeState: the range meter beside it (ac3mi_loudness_range_batch); nullptr: the plain meter
};
bool loudness_args_ok(const LoudnessLaunch &L);     // everything ac3mi_loudness_batch and _range_batch refuse, the context and the table apart
hipError_t launch_loudness(const LoudnessLaunch &L, hipStream_t stream);
hipError_t launch_loudness_read(const void *state, int n_streams, const double *tab, ac3mi_loudness_result *results, hipStream_t stream);
hipError_t launch_loudness_range_read(const void *range_state, int n_streams, const double *tab, ac3mi_loudness_range_result *results,
                                      hipStream_t stream);
hipError_t launch_loudness_words(const ac3mi_loudness_result *results, int n_streams, int frames_per_stream, uint32_t base_word,
                                 uint32_t *words, hipStream_t stream);

// truepeak.hip: the true-peak meter (ac3mi_truepeak_*; the rule is include/ac3mi.h's, its steps truepeak_rule.h's).  No table
// and no workspace in device memory
struct TruePeakLaunch {
    const int16_t *pcm;             // [S][F][1536][channels]
    int channels;
    uint8_t role[6];
    int n_streams, frames_per_stream;
    void *state;                    // [S] TruePeakState
};
bool truepeak_args_ok(const TruePeakLaunch &L);     // everything ac3mi_truepeak_batch refuses, the context apart
hipError_t launch_truepeak(const TruePeakLaunch &L, hipStream_t stream);
hipError_t launch_truepeak_read(const void *state, int n_streams, uint32_t ceiling_q28, ac3mi_truepeak_result *results, hipStream_t stream);

// limit.hip: the true-peak limiter (ac3mi_limit_*; the rule is include/ac3mi.h's, its steps limit_rule.h's).  No table and no
// workspace in device memory
struct LimitLaunch {
    const int16_t *pcm;             // [S][F][1536][channels]
    int16_t *out;                   // the same shape; pcm itself, or no overlap at all
    int channels;
    uint8_t role[6];
    uint32_t ceiling_q28, release_step_q24;
    int n_streams, frames_per_stream;
    void *state;                    // [S] LimitState
};
bool limit_args_ok(const LimitLaunch &L);   // everything ac3mi_limit_batch refuses, the context apart
hipError_t launch_limit(const LimitLaunch &L, hipStream_t stream);
hipError_t launch_limit_read(const void *state, int n_streams, ac3mi_limit_result *results, hipStream_t stream);

// resample.hip: the sample-rate converter (ac3mi_resample_*; the rule is include/ac3mi.h's, its steps resample_rule.h's).  tab: the
// pair's table on the device as resample_packed_table writes it on the host, [L][taps / 2] pairs of dwords
struct ResampleLaunch {
    int in_rate, out_rate, channels;
    const int16_t *pcm;             // [S][in_frames][1536][channels]
    int16_t *out;                   // [S][out_frames][1536][channels]; may be null when out_frames is 0
    int n_streams, in_frames, out_frames;
    void *state;                    // [S] ResampleState
    uint32_t *status;               // [S]
    const uint32_t *tab;
};
bool resample_args_ok(const ResampleLaunch &L);     // everything ac3mi_resample_batch refuses, the context and the table apart
// the pair's table in the kernel's form, L * taps dwords (null: only the count); 0: the pair's split does not pass its bound check
size_t resample_packed_table(int in_rate, int out_rate, uint32_t *h_tab);
hipError_t launch_resample(const ResampleLaunch &L, hipStream_t stream);

struct EncodeLaunch {
    EncConfig cfg;
    const int16_t *pcm;         // [S][F][1536][nch]
    int16_t *last;              // [S][nch][256]
    int32_t *csnr;              // [S]
    uint8_t *frames;            // [S][F][stride]
    int frame_stride, n_streams, frames_per_stream;
    uint8_t chmap[8];
    int32_t *ws_mdct;           // [S][F][6][nch][256]
    bool mdct_full_rows = false; // the rows are a stage tap: all 256 bins are stored, not only the coded ones
    uint8_t *ws_expo;           // [S][F][6][nch][256]
    int8_t *ws_shift;           // [S][F][6][nch]
    uint8_t *ws_eexp;           // [S][F][6][nch][256] encoded exponents
    int16_t *ws_emask;          // [S][F][6][nch][50]  masking curves minus the floor
    uint8_t *ws_strat;          // [S][F][6][nch]
    int32_t *ws_ebits;          // [S][F][nch]
    int32_t *ws_snr;            // [S][F][2] search results between the parts of the split pack kernel (may be null)
    uint32_t *ws_memo;          // [S][F][8] tabulated fit verdicts (may be null: the replay then costs everything itself)
    uint8_t *tap_eexp, *tap_bap, *tap_strat;
    int32_t *tap_snr;
    int32_t *tap_curve = nullptr;   // ac3mi_debug_search_curve: [S][F][1024][2], what the search costed (generic search kernel only)
    const int32_t *slot;
    int pack_mode = 0;          // ac3mi_set_encode_mode
    const uint32_t *search_hint = nullptr;     // transcode: per frame, an offset 16 csnroffst + fsnroffst near which to start costing (stride in dwords)
    int search_hint_stride = 0;
    uint8_t *ws_bsw = nullptr;  // [S][F][6][nch] block-switch decisions (ac3mi_set_encode_block_switch 1; null: long blocks only)
    uint8_t *ws_remat = nullptr;    // [S][F][6] rematrixing decisions (ac3mi_set_encode_rematrix 1; null, or not 2/0: none)
    int cpl_begf = -1;          // ac3mi_set_encode_coupling 1: cplbegf (0..12); -1: no coupling
    CplWs ws_cpl = {};          // its per-frame results (cpl_begf >= 0)
    int chbwcod = 50;           // ac3mi_set_encode_bandwidth: the call's chbwcod (0..50), nbc = 73 + 3 chbwcod
    bool bw = false;            // ... and whether it is on (mode 1 or 2): the runtime-bandwidth kernel variants run
    uint32_t bsi = BSI_DEFAULT; // ac3mi_set_encode_metadata, packed (bsi_word); not the default: the packers' MD variants run
    // ac3mi_set_encode_metadata_frames / _source: [S][F] raw words by the frame's position in the call (never by slot), coded
    // as bsi_sanitise(word) in place of `bsi`; frame f's dialnorm is also its DRC dialogue level.  Non-null: the MD variants run
    const uint32_t *bsi_words = nullptr;
    int drc_profile = 0;        // ac3mi_set_encode_drc: 1..5, 0 = no dynrng words
    int32_t *drc_state = nullptr;   // its smoothing state, [S] (or by slot)
    int16_t *ws_drc_gain = nullptr; // [S][F][6] static-curve gains (drc_profile > 0)
    uint8_t *ws_drc_code = nullptr; // [S][F][6] dynrng codes for the search and the packers
    int exp_strategy = 0;       // ac3mi_set_encode_exp_strategy: 1 = strategies by cost (the XS kernel variants), 0 = the reference's rule
    bool fixed_shape = true;    // ac3mi_set_fixed_shape: a 5.1 call may take the kernels with that shape compiled in (fixed51_shape)
    // ac3mi_set_encode_dynrng_frames / ac3mi_set_encode_drc_source, by the frame's position in the call (never by slot): the dynrng
    // code in force in every block, [S][F][6][2] (programme 0, 1), and the compr words, [S][F][2] (bit 8 compre, bits 0-7 compr).
    // Either non-null: the DW variants of the search and the packers run (never with drc_profile and dyn_codes together)
    const uint8_t *dyn_codes = nullptr;
    const uint16_t *compr_words = nullptr;
    const LaunchLog *log = nullptr;     // ac3mi_debug_launch_log: launch_stage appends what it launches (launch_rule.h); null: no tap
    const uint16_t *crc_rows = nullptr; // the packers' CRC table of cfg.frame_words on the device, [64][16] (crc_lanes.h: crcl_fill_rows); required
};
// carves CPL_FRAME_BYTES * nfr bytes at `base` into the arrays of CplWs (base 16-byte aligned)
CplWs cpl_slices(void *base, size_t nfr);
// carves cpl_remat_frame_bytes(nrow) * nfr bytes at `base` into the p* arrays of `w`
void cpl_remat_slices(CplWs &w, void *base, size_t nfr, int nrow = 2);
hipError_t launch_encode(const DeviceTables &tab, const EncodeLaunch &E, hipStream_t stream);
hipError_t launch_enc_history(const EncodeLaunch &E, hipStream_t stream);
void build_enc_tables(EncTables *t);
// 0 = rejected (AC3_encode_init returns 0).  acmod < 0: the reference's layout for the channel count ({1, 2, 3, 6, 7, 7},
// LFE with six channels); else acmod 0..7 with lfeon 0/1 (ac3mi_set_encode_layout 1), rejected unless channels is
// nfchans(acmod) + lfeon
int enc_config(int freq, int bitrate, int channels, EncConfig *c, int acmod = -1, int lfeon = 0);

hipError_t launch_convert_s16(const float *planes, int16_t *out, int flags, size_t n_blocks, hipStream_t stream);
int s16_channel_map(int flags, int map[6]);

void build_host_tables(float *window256, float2 *tw_long /*[8][16]*/, float2 *tw_short /*[8][16]*/);

// a device workspace: grown on demand (ws_grow in capi.hip), freed with the context
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    template <class T> T *at(size_t off = 0) const { return (T *)((uint8_t *)p + off); }
};

// the encoder's bitstream tools (ac3mi_set_encode_*); the defaults are the reference's fixed behaviour
struct EncTools {
    int block_switch = 0;               // ac3mi_set_encode_block_switch
    int rematrix = 0;                   // ac3mi_set_encode_rematrix
    int coupling = 0, cpl_begf = 0;     // ac3mi_set_encode_coupling
    int bw_mode = 0, bw_chbwcod = 50;   // ac3mi_set_encode_bandwidth
    uint32_t bsi = BSI_DEFAULT;         // ac3mi_set_encode_metadata (bsi_word)
    const uint32_t *bsi_words = nullptr;    // ac3mi_set_encode_metadata_frames
    int md_source = 0;                  // ac3mi_set_encode_metadata_source
    int drc_profile = 0;                // ac3mi_set_encode_drc
    int32_t *drc_state = nullptr;
    const uint8_t *dyn_codes = nullptr;     // ac3mi_set_encode_dynrng_frames
    const uint16_t *compr_words = nullptr;
    int drc_source = 0;                 // ac3mi_set_encode_drc_source
    int exp_strategy = 0;               // ac3mi_set_encode_exp_strategy
    int layout_mode = 0, layout_acmod = 0, layout_lfeon = 0;    // ac3mi_set_encode_layout
};

}  // namespace ac3mi

struct ac3mi_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // second stream: the byte-stream layer's PCIe copies beside the kernels (stream.hip)
    hipStream_t stream2 = nullptr;
    int encode_mode = 0;    // ac3mi_set_encode_mode
    ac3mi::EncTools tools;
    ac3mi::DeviceTables tab = {};
    // device workspaces
    ac3mi::DevBuf ws_coef;  // decode: coefficient planes between the front end and the transform
    ac3mi::DevBuf ws_blksw; // ... block-switch flags, then the per-frame surround-level-0 flags
    ac3mi::DevBuf ws_draws; // [S][F] draw counts + [S][F] u16 frame-start LFSR states (decode, frame-parallel)
    ac3mi::DevBuf ws_split; // descriptors, rows, coupling coordinates, generator positions between the split front end's kernels
    ac3mi::DevBuf ws_enc;   // encode: MDCT coefficients, exponents, block exponents between the kernels
    ac3mi::DevBuf ws_tc;    // transcode: s16 PCM between the decoder and the encoder
    ac3mi::DevBuf ws_bsw;   // block-switch decisions between the MDCT kernel and the packers, one byte per channel-block
    ac3mi::DevBuf ws_remat; // rematrixing decisions between the MDCT kernel, the search and the packers, one byte per frame-block
    ac3mi::DevBuf ws_cpl;   // coupling's per-frame workspace (ac3mi::CplWs, CPL_FRAME_BYTES a frame)
    ac3mi::DevBuf ws_cplr;  // with rematrixing on as well: cpl_remat_frame_bytes a frame
    ac3mi::DevBuf ws_drc;   // DRC gains and codes between the DRC kernels, the search and the packers, 3 bytes a frame-block
    ac3mi::DevBuf ws_crc;   // decode with ac3mi_set_decode_crc on: the CRC kernel's verdicts for the front end, one byte per frame
    ac3mi::DevBuf ws_bsi;   // transcode with ac3mi_set_encode_metadata_source 1: the BSI kernel's word per frame for the packers
    ac3mi::DevBuf ws_dyn;   // transcode with ac3mi_set_encode_drc_source 1: per frame the front end's raw words (24 bytes), the codes (12) and compr words (4)
    // every workspace above (ac3mi_destroy frees them, ac3mi_workspace_bytes sums them)
    template <class Ctx> static auto workspaces(Ctx *c)
    {
        return std::array{&c->ws_coef, &c->ws_blksw, &c->ws_draws, &c->ws_split, &c->ws_enc, &c->ws_tc,
                          &c->ws_bsw, &c->ws_remat, &c->ws_cpl, &c->ws_cplr, &c->ws_drc, &c->ws_crc, &c->ws_bsi, &c->ws_dyn};
    }
    // optional state-slot indirection for the next batch calls (ac3mi_set_state_slots)
    const int32_t *slots = nullptr;
    // optional liba52-exact overlap state around frames with surround level 0 (ac3mi_set_mix_state)
    float *mix_pending = nullptr;
    int32_t *mix_flags = nullptr;
    long long tile_frames = 131072;    // workspace bound: batches above this many frames go through in tiles of whole streams (0 = never)
    int decode_mode = 0;    // ac3mi_set_decode_mode
    int decode_crc = 0;     // ac3mi_set_decode_crc
    int fixed_shape = 1;    // ac3mi_set_fixed_shape
    int32_t *debug_search_curve = nullptr;  // ac3mi_debug_search_curve
    ac3mi::LaunchLog launch_log;            // ac3mi_debug_launch_log (host memory; words null: no tap)
    uint32_t *resample_tab[6] = {};  // ac3mi_resample_batch: a pair's table on the device, put there by the pair's first call, freed in ac3mi_destroy
    // the packers' CRC tables (crc_lanes.h), frame_words -> 2 KB on the device: put there when the context first meets the frame size, freed in ac3mi_destroy
    std::vector<std::pair<int, uint16_t *>> crc_rows;
    double *loud_tab = nullptr;     // ac3mi_loudness_*: bin edges and dialnorm thresholds on the device, put there by the first call (no workspace: it is a table)
    std::string err;
};
