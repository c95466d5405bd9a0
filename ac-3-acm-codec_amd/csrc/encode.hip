// encode.hip — AC-3 encoder on gfx950, bit-exact restatement of ENC/ac3enc.cpp (AC3_encode_frame, :1640-1763).
//
//  enc_mdct_kernel     one wavefront per (stream, frame, channel): gather/deinterleave via chmap, Q15 window,
//                      block-floating-point normalisation, the reference's 16-bit radix-2 DIT FFT in registers (one
//                      butterfly per lane and pass with exactly the reference's operands, shifts and int16
//                      truncations; lanes trade one point per pass), post-rotation, exponent extraction
//                      [ac3enc.cpp:1665-1722, 462-603]; then, still per channel (exp_stage): exponent strategy,
//                      min-merge over reuse runs, the +-2 constraint in closed form (enc_exp.h), band PSDs and masking curves of
//                      the blocks that send exponents                                   [ac3enc.cpp:606-761, 220-367]
//  enc_search_kernel   <1>: one wavefront per stream, frames in order (the SNR-offset search starts from the previous
//                      frame's csnroffst): the reference's exact search sequence replayed from exact verdicts, a window
//                      of sixteen consecutive offsets costed per sweep over the frame's run-start rows (snr_window.h);
//                      <3>: one wavefront per frame tabulates verdicts for few long streams, three offsets per sweep
//                                                                                       [ac3enc.cpp:764-975]
//  enc_packf_kernel    one wavefront per frame packs it: header, side information, exponent groups, the mantissas
//                      (enc_mant.h), both CRCs by per-lane chunk CRC + GF(2) combine    [ac3enc.cpp:1113-1638]
//  enc_packb_kernel    the same with a workgroup of six wavefronts per frame, one per audio block (small batches)
//  The frame's side-information syntax - the field lists both packers write through, the field accumulator, enc_packb_kernel's
//  closed-form counts and the search's price for the same fields - is enc_syntax.h's; here are the sink that puts the fields
//  into the LDS frame (PackSink) and the values each kernel feeds the lists.  enc_packf_kernel<FIXED51> without tools places
//  enc_syntax.h's images of the same fields by lanes instead (or_image, exp_row_at).
//
// Integer arithmetic only (no -ffast-math dependence); the Q15 tables come from the host (capi.hip)
// with the reference's expressions.
#include "ac3mi_internal.h"
#include "wave_ops.h"
#include "spec_tables.h"
#include "enc_mant.h"
#include "enc_syntax.h"
#include "enc_exp.h"
#include "snr_window.h"
#include "crc_lanes.h"
#include "mdct_rule.h"

#include <type_traits>

namespace ac3mi {

__device__ __forceinline__ int ilog2u(unsigned v) { return v ? 31 - __builtin_clz(v) : 0; }   // av_log2, :1539-1567

__device__ __forceinline__ int wave_sum(int v) { return (int)wave_sum_u32((uint32_t)v); }

// ---------------------------------------------------------------------------------------------
// kernel 2: exponent coding, bit allocation, quantisation, packing

struct PackParams {
    const int32_t *mdct;
    const uint8_t *eexp;        // [S][F][6][nch][256] encoded exponents   (exp_stage)
    const int16_t *emask;       // [S][F][6][nch][50]  masking curve minus the floor
    const uint8_t *strat;       // [S][F][6][nch]
    const int32_t *ebits;       // [S][F][nch] bits of the coded exponents
    const int8_t *shift;
    int32_t *csnr_state;        // [S] in/out
    const int32_t *slot;        // optional: stream s uses csnr_state[slot[s]]
    int32_t *snr;               // [S][F][2] csnroffst, fsnroffst between the parts of the split kernel
    uint32_t *memo;             // [S][F][8] tabulated fit verdicts (PART 3 -> PART 1): known_c, fits_c (64 bit each), known_f, fits_f, f_cc
    uint8_t *frames;            // [S][F][stride]
    const EncTables *tab;
    // taps (optional)
    uint8_t *tap_eexp;          // [S][F][6][nch][256]
    uint8_t *tap_bap;           // [S][F][6][nch][256]
    uint8_t *tap_strat;         // [S][F][6][nch]
    int32_t *tap_snr;           // [S][F][2]
    int32_t *tap_curve;         // [S][F][1024][2]: spare bits and ceiling sixths of every offset the search costed (ac3mi_debug_search_curve)
    int n_streams, frames_per_stream, frame_stride;
    int nch, nfbw, lfe, acmod, fscod, halfrate, bsid, frmsizecod, frame_words;
    int nbc;                    // coefficients per full-bandwidth channel (223)
    int chbwcod;
    // both CRC words by the lane rule (crc_lanes.h): the frame size's table in device memory, a row per lane, and its split
    const uint16_t *crc_rows;   // [64][16]: entry j of lane i's row = the lane's constant * x^j mod poly
    int crc_c, crc_n1;          // chunk bytes per lane; lanes of region 1
    int frw;                    // dwords of the frame buffer in (dynamic) LDS: the frame + 256 bytes of headroom, multiple of 4
    int marker;                 // the reference's "member already merged" value, 128 (:1375-1413); AC3MI_ENC_MARKER: test aid
    const uint32_t *hint;       // optional, [frame * hint_stride]: 16 csnroffst + fsnroffst the frame's SOURCE was coded with (transcode)
    int hint_stride;
    const uint8_t *bsw;         // optional, [S][F][6][nch]: blksw of each channel-block (block switching); null: all 0
    const uint8_t *remat;       // optional, [S][F][6]: 2/0 rematrixing, flags in bits 0-3, rematstr in bit 4; null: none
    CplWs cpl;                  // channel coupling (enc_cpl_kernel); cpl.word null: none
    int cpl_begf;
    int cpl_endf;               // cplendf of a coupled frame: 12, min(12, chbwcod >> 2) in the BW variants (cplendmant 73 + 12 cplendf)
    const uint8_t *drc;         // the DRC variants: [S][F][6] dynrng codes (enc_drc_smooth_kernel); null in the others
    uint32_t bsi;               // the MD packers: the BSI fields (bsi_word)
    const uint32_t *bsi_words;  // the MD packers: optional, [S][F] raw words by the frame's position in the call; frame f then codes bsi_sanitise(bsi_words[f])
    // the DW variants (ac3mi_set_encode_dynrng_frames / ac3mi_set_encode_drc_source), by the frame's position in the call:
    const uint8_t *dyn;         // optional, [S][F][6][2]: the dynrng code in force in each block, programme 0 and 1 (1: acmod 0 only)
    const uint16_t *compr;      // optional, [S][F][2]: bit 8 compre (compr2e), bits 0-7 compr (compr2)
};

// the BSI fields frame fidx codes (MD packers): the call's word, or the frame's own from the array (ac3mi_set_encode_metadata_frames /
// _source), sanitised here so that no array can make the packers write a reserved code.  Read where the header is written and
// nowhere else: a scalar load, nothing kept live across the frame
__device__ __forceinline__ uint32_t pack_bsi(const PackParams &P, size_t fidx)
{
    return P.bsi_words ? bsi_sanitise((uint32_t)__builtin_amdgcn_readfirstlane((int)P.bsi_words[fidx])) : P.bsi;
}

// dynrng words of a frame (ac3mi_set_encode_drc): block 0 sends its code, block b > 0 only when it differs from block b - 1's
__device__ __forceinline__ bool drc_sends(const uint8_t *code, int b) { return b == 0 || code[b] != code[b - 1]; }
// ... and of a frame's [6][2] codes in force (PackParams::dyn), per programme p: a frame starts at word 0 (gain 1.0) and a word
// holds to the frame's end, so block b sends iff its code differs from the one before it - block 0's from 0
__device__ __forceinline__ bool dyn_sends(const uint8_t *code, int b, int p) { return code[2 * b + p] != (b ? code[2 * b - 2 + p] : 0); }
// the frame's compr word of programme p (bit 8: sent), wave-uniform
__device__ __forceinline__ uint32_t compr_word(const PackParams &P, size_t fidx, int p)
{
    return P.compr ? (uint32_t)__builtin_amdgcn_readfirstlane((int)P.compr[fidx * 2 + p]) & 0x1ffu : 0u;
}

// the dynrng word programme p sends in block b of the frame, bit 8 = sent (the packers; enc_syntax.h's dynrng): the arrays' (DW
// with P.dyn: each programme's own code and sends), else the profile's - the same word for both programmes of dual mono
template <bool MD, bool DW>
__device__ __forceinline__ uint32_t pack_dynrng(const PackParams &P, size_t fidx, int b, int p)
{
    if constexpr (DW) if (P.dyn) return dyn_sends(P.dyn + fidx * 12, b, p) ? 0x100u | P.dyn[fidx * 12 + 2 * b + p] : 0u;
    if constexpr (MD) if (P.drc && drc_sends(P.drc + fidx * 6, b)) return 0x100u | P.drc[fidx * 6 + b];
    return 0u;
}

// tables of the PSD / masking-curve computation
struct MaskTabs {
    uint8_t latab[256];
    uint16_t hth[50];
    uint8_t band_of_bin[256];
    uint8_t band_start[52];
};

// The search kernel's LDS: the cost table and the list of run-start rows, and
// - the three-offset sweep (PART 3): the frame's 36 masking curves (+ 6 of a coupling row), read once per sweep and candidate;
// - the window sweep (PART 1; about one sweep per frame, the band lanes read their mask words from memory a row ahead): the
//   per-bin prefix sums a row's band lanes take their band sums from, and the per-block histogram of the bands' steps.
template <bool CPL>
struct SearchMaskRows {
    int16_t mask[CPL ? 42 : 36][50];       // masking curve minus the floor, row blk * nch + ch as exp_stage leaves them (a straight copy); 36 + blk: coupling
};
struct SearchWindowBufs {
    // [4 + bin]: inclusive prefix sum over the row's bins of one packed cost word ([3] = 0: a band's sum is [3 + end] - [3 + start])
    alignas(16) uint32_t scan[4 + 256];
    // [copy][b][t - 1][word]: what the bands whose k steps at offset g_lo + t (1..15) add to the wide words A, B (snr_window.h)
    // of the blocks b.., entered at the run's first block and taken back at the block behind its last (nothing to take back
    // behind block 5).  Four copies, lane & 3's: a row's fifty band lanes step at eight offsets t1 and at t1 + 8, so ten or
    // more of them would meet on one address, and LDS atomics on one address take their turns
    alignas(16) uint32_t hist[4][6][15][2];
};
template <bool CPL, bool WIN>
struct alignas(16) SearchLDS : std::conditional_t<WIN, SearchWindowBufs, SearchMaskRows<CPL>> {
    uint32_t bitlut[64];        // see "bap of one coefficient" below
    uint8_t strat[6][6];
    uint8_t band_of_bin[256];
    // the frame's run-start rows in (block, channel) order, for the search's sweeps: byte offset of the row's encoded
    // exponents (bits 0-13) | LFE row (7 coefficients, bit 14) | coupling row (bit 15: bins [cplstrtmant, 217) of the
    // coupling exponents) | blocks the run covers (bits 16-21) | coupled channel (bit 22: bins below cplstrtmant) | mask row (24-29)
    uint32_t rowdesc[CPL ? 42 : 36];
    // per band of the row being costed (two buffers: the next row's are worked out a row ahead), for each candidate offset:
    // 320 - max(0, ((mask - snroffset) >> 3) & ~3) as int16, so that a coefficient's table address x 4 is
    // clamp(term - 16 exponent, 0, 252); the window sweep: the same for the window's first offset, + 4 and + 8 (win_term)
    uint2 terms[2][50];
};

// put_bits (:148-176).  `v` may be wider than n bits (the release build does not mask it): the excess is OR-ed onto
// the bits before the field as far as the 32-bit word it starts in, which is what the 64-bit shift below does.
__device__ __forceinline__ void put_bits(uint32_t *fr, int frw, uint32_t pos, int n, uint32_t v)
{
    if (n <= 0) return;
    const uint32_t w = pos >> 5;
    if (w + 1 >= (uint32_t)frw) return;
    const uint64_t x = (uint64_t)v << (64 - n - (pos & 31));
    const uint32_t hi = (uint32_t)(x >> 32), lo = (uint32_t)x;
    if (hi) atomicOr(&fr[w], hi);
    if (lo) atomicOr(&fr[w + 1], lo);
}

// row `row` of a block's exponent dwords (no indexing of the register array), `other` for any row but 0..5
__device__ __forceinline__ uint32_t pick_row(const uint32_t (&ew)[6], int row, uint32_t other)
{
    uint32_t dw = other;
#pragma unroll
    for (int c2 = 0; c2 < 6; c2++) dw = c2 == row ? ew[c2] : dw;
    return dw;
}

// The packers' sink of enc_syntax.h's field lists: the accumulator's bits reach the LDS frame from lane 0, and `flush` empties
// it before the lanes write at `pos` themselves (exponent groups, mantissas).  One per stretch of fields that starts and ends
// flushed - the header, each block - from the frame's bit `at`.  row_of(row): the lane's dword (four bins) of a row's encoded
// exponents, row SYN_CPL the coupling row's, whose exponents start at bin `cs`.
template <class Row>
struct PackSink : SynWriter<PackSink<Row>> {
    uint32_t *fr;
    int frw, lane;
    uint8_t *erow;                      // 256 bytes of LDS: the encoded exponents of the row whose groups are being packed
    Row row_of;
    int cs;
    __device__ __forceinline__ PackSink(uint32_t *fr_, int frw_, int lane_, uint8_t *erow_, Row row_of_, int cs_, uint32_t at)
        : fr(fr_), frw(frw_), lane(lane_), erow(erow_), row_of(row_of_), cs(cs_) { this->pos = at; }
    __device__ __forceinline__ void store(uint32_t at, int n, uint32_t v) { if (lane == 0) put_bits(fr, frw, at, n, v); }
    // a row's exponents: the absolute exponent (the coupling row's: bin cs - 1 holds 2 cplabsexp), then lanes over the ng groups.
    // (tests/enc_syntax_c's HostSink::exponents mirrors the put(4) - flush - groups sequence: the 64-bit bound it proves
    // holds here as long as the two keep the same flush)
    __device__ __forceinline__ void exponents(int row, int strat, int ng)
    {
        const int gs = syn_grpsize(strat), first = row == SYN_CPL ? cs : 1;
        const uint8_t *e = erow;
        const uint32_t dw = row_of(row);
        wave_sync();                                                // the previous row's groups have read the row
        *reinterpret_cast<uint32_t *>(&erow[4 * lane]) = dw;
        wave_sync();
        this->put(4, (uint32_t)__builtin_amdgcn_readfirstlane((int)e[first - 1]) >> (row == SYN_CPL ? 1 : 0));
        this->flush();
        for (int g = lane; g < ng; g += 64) {
            const int k0 = first + 3 * g * gs;
            const int prev = g ? e[k0 - gs] : e[first - 1];
            const int d0 = e[k0] - prev + 2, d1 = e[k0 + gs] - e[k0] + 2, d2 = e[k0 + 2 * gs] - e[k0 + gs] + 2;
            put_bits(fr, frw, this->pos + 7 * g, 7, (uint32_t)((d0 * 5 + d1) * 5 + d2));
        }
        this->pos += 7 * ng;
    }
};

// The same for a frame whose side information comes as images (enc_syntax.h: SynImages51).
// A two-dword image w[0] : w[1] into the frame from bit `at`: lanes 0..2 OR a dword each (syn_image_dword).  Dwords that would
// start within the last two of the buffer are dropped, as put_bits drops a field there: 256 bytes behind the frame's last byte.
__device__ __forceinline__ void or_image(uint32_t *fr, int frw, const uint32_t *w, uint32_t at, int lane)
{
    if (lane < 3) {
        const uint32_t d = syn_image_dword(w[0], w[1], lane, at), i = (at >> 5) + (uint32_t)lane;
        if (d && i + 1 < (uint32_t)frw) atomicOr(&fr[i], d);
    }
}
// A row's exponents from bit `at`: PackSink::exponents of a channel row without the accumulator - the lane of group 0 writes
// the absolute exponent in front of it, as one field of 11 bits.
__device__ __forceinline__ void exp_row_at(uint32_t *fr, int frw, uint8_t *erow, uint32_t dw, uint32_t at, int strat, int ng, int lane)
{
    const int gs = syn_grpsize(strat);
    const uint8_t *e = erow;
    wave_sync();                                                    // the previous row's groups have read the row
    *reinterpret_cast<uint32_t *>(&erow[4 * lane]) = dw;
    wave_sync();
    for (int g = lane; g < ng; g += 64) {
        const int k0 = 1 + 3 * g * gs;
        const int prev = g ? e[k0 - gs] : e[0];
        const int d0 = e[k0] - prev + 2, d1 = e[k0 + gs] - e[k0] + 2, d2 = e[k0 + 2 * gs] - e[k0 + gs] + 2;
        const uint32_t code = (uint32_t)((d0 * 5 + d1) * 5 + d2);
        put_bits(fr, frw, g ? at + 4 + 7 * g : at, g ? 7 : 11, g ? code : ((uint32_t)e[0] << 7) | code);
    }
}

// ---------------------------------------------------------------------------------------------
// exp_stage's routines, wavefront-wide.

// per byte (values < 128): b's byte where it is smaller and `where` selects the byte, else a's
__device__ __forceinline__ uint32_t bytes_min_where(uint32_t a, uint32_t b, uint32_t where)
{
    const uint32_t ge = (((a | 0x80808080u) - b) >> 7) & 0x01010101u;       // 1: a >= b (no borrow crosses a byte)
    const uint32_t m = ((ge << 8) - ge) & where;            // ge * 0xff without the quarter-rate v_mul_lo_u32
    return (b & m) | (a & ~m);
}

// encode_exp (:684-761) on one 256-byte row in LDS, a dword per lane: the lane's entries (chan_exp_entries) under the +-2 delta
// constraint (exp_constrain, both enc_exp.h), written back to the bins they cover, bin 0 with them.  Returns the set's bits.
// PER = entries per lane, a compile-time constant per strategy (D15 4, D25 2, D45 1): a reuse-poor frame (decoded audio
// re-encoded sends 24 sets, most of them D45 / D25) spends its exponent stage here, and the coarse strategies need a quarter /
// half of the per-entry work.
template <int PER>
__device__ __forceinline__ int encode_exp_wave_t(uint8_t *row, int n, int lane)
{
    const int groups = syn_exp_groups(n, exp_strategy_of<PER>), ng = 3 * groups;
    uint32_t *q = reinterpret_cast<uint32_t *>(row);
    const uint32_t own = q[lane], nxt = q[lane + 1];        // lane 63 reads the dword behind the row: entries beyond ng, never used
    int bin[4], g[PER], ix[PER];
    bool valid[PER];
    const int row0 = chan_exp_entries<PER>(own, nxt, ng, lane, bin, g, ix, valid);
    const int head = exp_constrain<PER, true>(g, ix, valid, row0, lane);
    const int row0new = head < row0 ? head : row0;
    // back to bins, 4 / PER of them an entry (entries beyond ng leave their bins alone)
    uint32_t o = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) o |= (uint32_t)(valid[k * PER / 4] ? g[k * PER / 4] : bin[k]) << (8 * k);
    const uint32_t prev = (uint32_t)__builtin_amdgcn_update_dpp(row0new << 24, (int)o, 0x138, 0xf, 0xf, false);
    q[lane] = __builtin_amdgcn_alignbyte(o, prev, 3u);
    return 4 + 7 * groups;
}

__device__ int encode_exp_wave(uint8_t *row, int n, int strategy, int lane)
{
    if (strategy == 1) return encode_exp_wave_t<4>(row, n, lane);
    if (strategy == 2) return encode_exp_wave_t<2>(row, n, lane);
    return encode_exp_wave_t<1>(row, n, lane);
}

// encode_exp_wave_t<PER> in registers, for the cost of a candidate set (ac3mi_set_encode_exp_strategy 1): `own` is this lane's
// dword of the row (bins 4 lane .. 4 lane + 3); returns this lane's share of the sum of the coded exponents over bins [0, n),
// bin 0 on lane 0.  The row is not written.
template <int PER>
__device__ __forceinline__ int encode_exp_sum_t(uint32_t own, int n, int lane)
{
    constexpr int gs = 4 / PER;
    const int ng = 3 * syn_exp_groups(n, exp_strategy_of<PER>);
    const uint32_t nxt = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)own, 0x130, 0xf, 0xf, false);      // wave_shl:1
    int bin[4], g[PER], ix[PER];
    bool valid[PER];
    const int row0 = chan_exp_entries<PER>(own, nxt, ng, lane, bin, g, ix, valid);
    const int head = exp_constrain<PER, true>(g, ix, valid, row0, lane);
    int sum = lane == 0 ? (head < row0 ? head : row0) : 0;
#pragma unroll
    for (int c = 0; c < PER; c++) {
        int cnt = n - (4 * lane + 1 + c * gs);                  // bins of entry c below n
        cnt = cnt < 0 ? 0 : cnt > gs ? gs : cnt;
        sum += valid[c] ? g[c] * cnt : 0;
    }
    return sum;
}

// cpl_encode_exp's coded exponents summed over [cs, ce) (this lane's share), the row in LDS left as it is
__device__ __forceinline__ int cpl_exp_sum(const uint8_t *row, int cs, int ce, int strategy, int lane)
{
    const int gs = syn_grpsize(strategy);
    int g[3], ix[3];
    bool valid[3];
    cpl_exp_entries(row, cs, 3 * syn_cpl_exp_groups(cs, ce, strategy), gs, lane, g, ix, valid);
    exp_constrain<3, false>(g, ix, valid, 0, lane);
    int sum = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) sum += valid[c] ? g[c] * gs : 0;
    return sum;
}

// Exponent strategies by cost (ac3mi_set_encode_exp_strategy 1; the rule is include/ac3mi.h's).  E[b]: block b's raw row in
// LDS; `in`: this lane's byte mask of the coded range - [0, n) of a channel, [cs, ce) of the coupling row (CPLROW: the
// candidate's merged row goes through `scratch`, a 256-byte LDS row, since the coupling groups straddle lanes); `extra`: the
// set's bits besides absexp and the groups (gainrng 2 + chbwcod 6, gainrng 2 in a coupled frame, 0 for the LFE and the
// coupling row); `d15`: D15 only (the LFE).  A candidate (i, L, s) costs bits(s) + sum over its blocks and the range of
// (raw - coded) = bits(s) + sum_b R_b - L sum c: per lane the raw sum (v_sad_u8) and the three strategies' coded sums, two
// sums per wave reduction (each is below 2^16).  J(i) = min over L, s of cost(i, L, s) + J(i + L), wave-uniform; the loops stay
// rolled (one copy of the three encode_exp sums) and J, the choices live in scalars.  Returns block b's strategy in bits
// 4b .. 4b + 3 (0: reuse).
template <bool CPLROW>
__device__ uint32_t xs_choose(const uint8_t (*E)[256], uint8_t *scratch, uint32_t in, int n, int cs, int ce, int extra,
                              bool d15, int lane)
{
    int bits[3];
#pragma unroll
    for (int s = 0; s < 3; s++) bits[s] = 4 + 7 * (CPLROW ? syn_cpl_exp_groups(cs, ce, s + 1) : syn_exp_groups(n, s + 1)) + extra;
    int J1 = 0, J2 = 0, J3 = 0, J4 = 0, J5 = 0, J6 = 0;         // J(1) .. J(6) (J(6) = 0)
    uint32_t choice = 0;                                        // per block i: L | s << 3, 5 bits each
#pragma unroll 1
    for (int i = 5; i >= 0; i--) {
        uint32_t acc = *reinterpret_cast<const uint32_t *>(&E[i][4 * lane]);
        uint32_t racc = 0;
        int best = 0x7fffffff, bl = 1, bs = 1;
#pragma unroll 1
        for (int L = 1; L <= 6 - i; L++) {
            const uint32_t rb = *reinterpret_cast<const uint32_t *>(&E[i + L - 1][4 * lane]);
            if (L > 1) acc = bytes_min_where(acc, rb, in);
            racc = __builtin_amdgcn_sad_u8(rb & in, 0u, racc);
            int c15, c25 = 0, c45 = 0;
            if constexpr (CPLROW) {
                *reinterpret_cast<uint32_t *>(&scratch[4 * lane]) = acc;
                wave_sync();
                c15 = cpl_exp_sum(scratch, cs, ce, 1, lane);
                c25 = cpl_exp_sum(scratch, cs, ce, 2, lane);
                c45 = cpl_exp_sum(scratch, cs, ce, 3, lane);
                wave_sync();
            } else {
                c15 = encode_exp_sum_t<4>(acc, n, lane);
                if (!d15) {
                    c25 = encode_exp_sum_t<2>(acc, n, lane);
                    c45 = encode_exp_sum_t<1>(acc, n, lane);
                }
            }
            const uint32_t a = wave_sum_u32((uint32_t)c15 | (uint32_t)c25 << 16);
            const uint32_t b = wave_sum_u32((uint32_t)c45 | racc << 16);
            const int R = (int)(b >> 16);
            const int k = i + L;
            const int Jn = k == 1 ? J1 : k == 2 ? J2 : k == 3 ? J3 : k == 4 ? J4 : k == 5 ? J5 : J6;
            const int C[3] = {(int)(a & 0xffffu), (int)(a >> 16), (int)(b & 0xffffu)};
#pragma unroll
            for (int s = 0; s < 3; s++) {
                if (s > 0 && d15) break;
                const int cost = bits[s] + R - L * C[s] + Jn;
                if (cost < best) { best = cost; bl = L; bs = s + 1; }
            }
        }
        J1 = i == 1 ? best : J1; J2 = i == 2 ? best : J2; J3 = i == 3 ? best : J3;
        J4 = i == 4 ? best : J4; J5 = i == 5 ? best : J5;
        choice |= (uint32_t)(bl | bs << 3) << (5 * i);
    }
    uint32_t st = 0;
    for (int i = 0; i < 6;) {
        const int c = (int)((choice >> (5 * i)) & 31u);
        st |= (uint32_t)(c >> 3) << (4 * i);
        i += c & 7;
    }
    return st;
}

// The two masking-curve routines' common parts, one lane per band b (:259-367).
// The fast / slow leaks at band b from the `live` bands up to it: prefix maxima of psd - gain + band * decay (two scans
// interleaved, wave_ops.h), taken back by b * decay
__device__ __forceinline__ void mask_leaks(int psd, bool live, int b, int sdecay, int fdecay, int sgain, int fgain, int &fast, int &slow)
{
    constexpr int NEG = -0x3fffffff;
    fast = live ? psd - fgain + b * fdecay : NEG;
    slow = live ? psd - sgain + b * sdecay : NEG;
    wave_incl_scan_max2(fast, slow);
    fast -= b * fdecay;
    slow -= b * sdecay;
}
// ... and what follows the excitation: the knee's correction, the hearing threshold, and the store - 0 in a band outside the row
__device__ __forceinline__ void mask_store(const MaskTabs &T, int16_t *mask, int b, bool inside, int excite, int psd, int dbknee, int halfrate)
{
    const int t = dbknee - psd;
    if (t > 0) excite += t >> 2;
    const int h = T.hth[(b < 50 ? b : 49) >> halfrate];
    if (b < 50) mask[b] = inside ? (int16_t)(excite > h ? excite : h) : (int16_t)0;
}

// Masking curve of one row, one lane per band (:220-367).  bndpsd[] must hold the band PSDs.
//  * lowcomp is a reset-or-decrement automaton: value = max(0, R(last reset) - 64 * decrements since)
//  * the leaks are seeded at band begin-1
__device__ void mask_row_wave(const MaskTabs &T, int16_t *bndpsd, int bndend, bool is_lfe, int sdecay, int fdecay, int sgain,
                              int dbknee, int fgain, int halfrate, int lane)
{
    constexpr int NEG = -0x3fffffff;
    const int b = lane;
    const int cur = b < bndend ? bndpsd[b] : 0;
    const int nxt = (b + 1 < bndend && !(is_lfe && b == 6)) ? bndpsd[b + 1] : 0;
    const bool skip = (is_lfe && b == 6) || b >= 22 || b >= bndend;
    const bool reset = !skip && b < 20 && cur + 256 == nxt;
    const int dec = skip || reset ? 0 : b >= 20 ? 2 : (cur > nxt ? 1 : 0);
    const int D = (int)wave_incl_scan_u32((uint32_t)dec);
    const int rix = wave_incl_scan_max(reset ? b : NEG);
    const int Dr = __shfl(D, rix < 0 ? 0 : rix, 64);
    int lowcomp = 0;
    if (rix >= 0) { lowcomp = (rix < 7 ? 384 : 320) - 64 * (D - Dr); lowcomp = lowcomp < 0 ? 0 : lowcomp; }

    const bool stop = b >= 2 && b < 7 && b < bndend && !(is_lfe && b == 6) && cur <= nxt;
    const unsigned long long sm = __ballot(stop);
    const int begin = sm ? __builtin_ctzll(sm) + 1 : 7;
    const bool live = b >= begin - 1 && b < bndend;
    int fast, slow;
    mask_leaks(cur, live, b, sdecay, fdecay, sgain, fgain, fast, slow);
    int excite;
    if (b < begin) excite = (int16_t)(cur - fgain - lowcomp);
    else if (b < 22) { const int v = fast - lowcomp; excite = (int16_t)(slow > v ? slow : v); }
    else excite = (int16_t)(fast > slow ? fast : slow);
    mask_store(T, bndpsd, b, b < bndend, excite, cur, dbknee, halfrate);
}

// ---------------------------------------------------------------------------------------------
// second half of kernel 1: exponent strategy, min-merge, constraint and masking curves.  Everything here is
// independent per channel, like the MDCT: the wavefront that transformed the six blocks of one
// (stream, frame, channel) goes straight on with their exponents.

struct ExpParams {
    uint8_t *eexp;              // [S][F][6][nch][256] encoded exponents
    int16_t *emask;             // [S][F][6][nch][50]
    uint8_t *strat;             // [S][F][6][nch]
    int32_t *ebits;             // [S][F][nch]
    const EncTables *tab;
    int nch, lfe, fscod, halfrate, nbc;
};

struct ExpLDS {
    uint8_t E[6][256];
    int16_t mask[6][50];
    MaskTabs t;
    uint8_t strat[8];
};

// Runs at the end of enc_mdct_kernel: L.t holds the tables, L.E the six blocks' raw exponents of this channel.
// KEEP (enc_cpl_kernel, a coupled channel): the strategies are the ones P.strat already holds (mode 0's, from all 256 bins),
// the rest is recomputed for the P.nbc = cplstrtmant bins the channel codes.
// XS (ac3mi_set_encode_exp_strategy 1): the strategies are xs_choose's over the coded bins [0, n); 1: a set also sends
// gainrng and chbwcod (enc_mdct_kernel), 2: gainrng only (a coupled channel, enc_cpl_kernel).
// FX (enc_mdct_kernel's fixed 5.1 shape): six channels, the last the LFE, 223 coefficients - constants instead of P's.
template <bool KEEP = false, int XS = 0, bool FX = false>
__device__ void exp_stage(const ExpParams &P, ExpLDS &L, size_t fidx, int ch, int lane)
{
    const int nch = FX ? 6 : P.nch;
    const bool is_lfe = (FX || P.lfe) && ch == nch - 1;
    const int n = is_lfe ? 7 : FX ? 223 : P.nbc;
    uint32_t raw[6];
#pragma unroll
    for (int b = 0; b < 6; b++) raw[b] = *reinterpret_cast<const uint32_t *>(&L.E[b][4 * lane]);
    uint32_t below = 0;                                         // this lane's bytes of bins below n
#pragma unroll
    for (int c = 0; c < 4; c++) below |= (4 * lane + c < n ? 0xffu : 0u) << (8 * c);

    // ---- exponent strategy (:617-669): sum of |differences| over all 256 bins against the block before (two sums per
    //      reduction: each stays below 2^16) ----
    int st[6];
    st[0] = 1;
    if constexpr (KEEP) {
#pragma unroll
        for (int b = 0; b < 6; b++) st[b] = (int)P.strat[(fidx * 6 + b) * nch + ch];
    } else if constexpr (XS != 0) {
        const uint32_t x = xs_choose<false>(L.E, nullptr, below, n, 0, 0, is_lfe ? 0 : XS == 1 ? 8 : 2, is_lfe, lane);
#pragma unroll
        for (int b = 0; b < 6; b++) st[b] = (int)((x >> (4 * b)) & 15u);
    } else {
        const uint32_t d1 = __builtin_amdgcn_sad_u8(raw[1], raw[0], 0u), d2 = __builtin_amdgcn_sad_u8(raw[2], raw[1], 0u);
        const uint32_t d3 = __builtin_amdgcn_sad_u8(raw[3], raw[2], 0u), d4 = __builtin_amdgcn_sad_u8(raw[4], raw[3], 0u);
        const uint32_t d5 = __builtin_amdgcn_sad_u8(raw[5], raw[4], 0u);
        const uint32_t t12 = wave_sum_u32(d1 | d2 << 16), t34 = wave_sum_u32(d3 | d4 << 16), t5 = wave_sum_u32(d5);
        st[1] = (t12 & 0xffffu) > 1000u; st[2] = (t12 >> 16) > 1000u;
        st[3] = (t34 & 0xffffu) > 1000u; st[4] = (t34 >> 16) > 1000u;
        st[5] = t5 > 1000u;
    }
    uint32_t starts = 0;                                        // bit b: block b sends exponents (wave-uniform)
#pragma unroll
    for (int b = 0; b < 6; b++) starts |= (st[b] != 0 ? 1u : 0u) << b;
    if (!KEEP && XS == 0 && !is_lfe) {
#pragma unroll
        for (int b = 0; b < 6; b++) {
            if (st[b] == 0) continue;
            int run = 1;                                                // blocks until the next new set
#pragma unroll
            for (int e = 1; e < 6; e++) if (b + e < 6 && run == e && st[b + e] == 0) run = e + 1;
            st[b] = run == 1 ? 3 : run <= 3 ? 2 : 1;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int b = 0; b < 6; b++) L.strat[b] = (uint8_t)st[b];
    }

    // ---- min-merge over reuse runs (:1731-1737), bins below n only: in registers, four bins per lane ----
#pragma unroll
    for (int b = 0; b < 5; b++) {
        if (!((starts >> b) & 1u)) continue;
        bool open = true;
        bool touched = false;
#pragma unroll
        for (int e = b + 1; e < 6; e++) {
            open = open && !((starts >> e) & 1u);
            if (open) { raw[b] = bytes_min_where(raw[b], raw[e], below); touched = true; }
        }
        if (touched) *reinterpret_cast<uint32_t *>(&L.E[b][4 * lane]) = raw[b];
    }
    wave_sync();

    // ---- encode_exp on run starts (:1739-1746); the blocks of a run are sent the start's exponents ----
    int exp_bits = 0;
    for (uint32_t m = starts; m; m &= m - 1) {
        const int b = __builtin_ctz(m);
        exp_bits += encode_exp_wave(L.E[b], n, L.strat[b], lane);
    }
    wave_sync();
    {
        uint32_t cur = 0;
        for (int b = 0; b < 6; b++) {
            if ((starts >> b) & 1u) cur = *reinterpret_cast<const uint32_t *>(&L.E[b][4 * lane]);
            *reinterpret_cast<uint32_t *>(P.eexp + ((fidx * 6 + b) * nch + ch) * 256 + 4 * lane) = cur;
        }
    }

    // ---- band PSDs (:220-258) and masking curves (:259-367) of the blocks that send exponents; a block that
    //      reuses them has the same curve.  Bands 0..27 are single bins; the 22 wider ones are integrated by
    //      one lane each, two rows per sweep ----
    {
        const int nsingle = n < 28 ? n : 28;
        for (uint32_t m = starts; m; m &= m - 1) {
            const int r = __builtin_ctz(m);
            if (lane < nsingle) L.mask[r][lane] = (int16_t)(3072 - ((int)(int8_t)L.E[r][lane] << 7));
        }
        if (n > 28) {
            // Ten lanes per row, six rows in ONE sweep of 23 steps: a lane integrates a stretch of equally wide bands one after
            // the other (bands 28..49 start at 28 31 .. 46 | 49 55 .. 79 | 85 97 109 121 | 133 157 181 205 229): slots 0-4 a
            // 24-bin band each, 5-6 two 12-bin bands, 7 four and 8 two 6-bin bands, 9 the seven 3-bin bands - at most 24 bins.
            const int r = (lane * 205) >> 11, slot = lane - 10 * r;                 // lane / 10, lane % 10
            const int fb = slot < 5 ? 45 + slot : slot == 5 ? 41 : slot == 6 ? 43 : slot == 7 ? 35 : slot == 8 ? 39 : 28;
            const int nb = slot < 5 ? 1 : slot < 7 ? 2 : slot == 7 ? 4 : slot == 8 ? 2 : 7;
            const int lw = slot < 5 ? 3 : slot < 7 ? 2 : slot < 9 ? 1 : 0;          // bands of 3 << lw bins
            const bool rowon = lane < 60 && ((starts >> r) & 1u);
            const int rr = rowon ? r : 0;
            const int start = L.t.band_start[fb];
            int end1 = L.t.band_start[fb + nb];
            end1 = end1 < n ? end1 : n;
            const int len = rowon ? end1 - start : 0;                               // bins of the stretch inside the channel
            // the stretch's exponents: seven dwords of the row, shifted so that byte 0 is its first bin; the sweep's only
            // dependent LDS access per step is then the log-add table (as in the decoder's bit allocation, decode_common.h)
            const uint32_t *q = reinterpret_cast<const uint32_t *>(&L.E[rr][start & ~3]);
            uint32_t dw[7], ab[6];
#pragma unroll
            for (int i = 0; i < 7; i++) dw[i] = q[i];
#pragma unroll
            for (int i = 0; i < 6; i++) ab[i] = __builtin_amdgcn_alignbyte(dw[i + 1], dw[i], (uint32_t)start & 3u);
            int16_t *mrow = &L.mask[rr][fb];
            const bool r3 = lw == 0, r6 = lw <= 1, r12 = lw <= 2;
            int v = 3072 - ((int)(ab[0] & 0xffu) << 7);
#pragma unroll
            for (int j = 1; j < 24; j++) {
                const int pj = 3072 - ((int)((ab[j >> 2] >> (8 * (j & 3))) & 0xffu) << 7);
                // |v - pj| in one v_sad_u16 and the larger of the two in one v_max (both are 0 .. 2^15 here: exponents are
                // 0 .. 24 and a band's sum stays below 3072 + 23 x 64; hipcc spent seven instructions on the two)
                int t = (int)(__builtin_amdgcn_sad_u16((uint32_t)v, (uint32_t)pj, 0u) >> 1);
                t = t > 255 ? 255 : t;
                int nv = (v > pj ? v : pj) + (int)L.t.latab[t];
                if (j % 3 == 0) {                                                   // a band may end here
                    const bool ends = j % 12 == 0 ? r12 : j % 6 == 0 ? r6 : r3;
                    if (ends && j < len) mrow[((j / 3) >> lw) - 1] = (int16_t)v;
                    nv = ends ? pj : nv;
                }
                v = j < len ? nv : v;
            }
            if (len > 0) mrow[((((uint32_t)(len - 1)) * 0xaaabu) >> 17) >> lw] = (int16_t)v;
        }
        wave_sync();
        // fixed allocation codes (:861-879)
        const int sdecaycod = 2, fdecaycod = 1, fgaincod = 4;
        constexpr int sgaincod = 1, dbkneecod = 2;
        const int sdecay = enc_sdecay(sdecaycod) >> P.halfrate, fdecay = enc_fdecay(fdecaycod) >> P.halfrate;
        const int sgain = enc_sgain(sgaincod), dbknee = enc_dbknee(dbkneecod), fgain = enc_fgain(fgaincod);
        const int bndend = L.t.band_of_bin[n - 1] + 1;
        for (uint32_t m = starts; m; m &= m - 1)
            mask_row_wave(L.t, L.mask[__builtin_ctz(m)], bndend, is_lfe, sdecay, fdecay, sgain, dbknee, fgain, P.halfrate, lane);
    }
    wave_sync();

    // ---- results: the pack kernel wants the masks minus the floor (floorcod 4: 0x1f0); a block inside a run has its start's
    //      curve.  Two rows of 25 dwords per step ----
    static_assert(enc_floor(4) == 0x1f0 && enc_sgain(1) == 0x4d8 && enc_dbknee(2) == 0x900, "ENC/ac3tab.h:151-161");
    {
        typedef short short2v __attribute__((ext_vector_type(2)));
        const int half = lane >= 25 ? 1 : 0, k2 = lane - 25 * half;
        int src[6];
        src[0] = 0;
#pragma unroll
        for (int b = 1; b < 6; b++) src[b] = ((starts >> b) & 1u) ? b : src[b - 1];
#pragma unroll
        for (int it = 0; it < 3; it++) {
            const int b = 2 * it + half, sr = half ? src[2 * it + 1] : src[2 * it];
            if (lane < 50) {
                short2v v = *reinterpret_cast<const short2v *>(&L.mask[sr][2 * k2]);
                v -= (short2v){(short)enc_floor(4), (short)enc_floor(4)};
                *reinterpret_cast<short2v *>(P.emask + ((fidx * 6 + b) * nch + ch) * 50 + 2 * k2) = v;
            }
        }
    }
    if (lane < 6) P.strat[(fidx * 6 + lane) * nch + ch] = L.strat[lane];
    if (lane == 0) P.ebits[fidx * nch + ch] = exp_bits;
}

// ---------------------------------------------------------------------------------------------
// kernel 1: window + normalise + MDCT + exponents

struct MdctParams {
    const int16_t *pcm;         // [S][F][1536][nch] interleaved
    int16_t *last;              // [S][nch][256] history before frame 0 (rewritten here when store_history)
    int32_t *mdct;              // [S][F][6][nch][256]
    uint8_t *expo;              // [S][F][6][nch][256]
    int8_t *shift;              // [S][F][6][nch]
    const EncTables *tab;
    int n_streams, frames, nch;
    uint8_t chmap[8];
    const int32_t *slot;        // optional: stream s keeps its history in slot[s] (stride 6*256 samples)
    int store_history;          // one frame per stream: this kernel also leaves the new history (else enc_history_kernel)
    int full_rows;              // store all 256 coefficients of a row (stage tap); else only the bins the packer codes
    uint8_t *bsw;               // enc_mdct_kernel<true, *>: [S][F][6][nch] block-switch decisions for the packers
    ExpParams x;                // the exponent stage that follows the transform
    uint8_t *remat;             // enc_mdct_kernel<*, true>: [S][F][6] rematrixing decisions for the search and the packers
};

#ifndef ENC_MDCT_LB
#define ENC_MDCT_LB 7        // 71 VGPRs, no scratch: 1.97 ms against 2.00 at 5 or 6 (75 VGPRs) and 2.07 at 8 (64 VGPRs, 24 bytes of scratch)
#endif
#ifndef ENC_MDCT_BSW_LB
#define ENC_MDCT_BSW_LB 5    // block switching: 95 VGPRs, no scratch (at 6: 80 VGPRs and 64 bytes of scratch, at 7: 100 bytes)
#endif
// Block switching (BSW, ac3mi_set_encode_block_switch 1).  Per block, before the window: the transient detector of
// include/ac3mi.h on the raw samples (z = the 256 old || the 256 new ones, through LDS: lane L takes the second differences
// of z[8L .. 8L+7], groups of eight lanes the 64-sample segments), a wave-uniform verdict.  A switched block keeps the window
// and the block-floating-point shift of its 512 samples and takes A/52's pair of 256-point transforms instead of the
// 512-point one, restated like the long one at N = 256 (ac3enc.cpp:574-603 with MDCT_N = 256): transform 1 is that MDCT of
// the samples rotated by N/4 (phase term 0: alpha = -1), transform 2 of the samples rotated by 3N/4 (alpha = +1).  Each is
// a 64-point complex FFT: lanes 0-31 hold transform 1, lanes 32-63 transform 2, lane l of a half points bitrev5(l) and
// bitrev5(l) + 32 - the long layout one level down, so passes 0..5 are the long passes 0..5 with the same twiddles (the
// 64-point table is every other entry of the 128-point one) and trades at distances 1..16 that never cross the halves.
// coef[2k] = X1[k], coef[2k+1] = X2[k], the layout liba52's a52_imdct_256 reads: same scale as the long path.
//
// Rematrixing (REMAT, ac3mi_set_encode_rematrix 1, 2/0 only).  A stereo frame is one workgroup of two wavefronts, wave w
// = channel w, each with its own row and exponent LDS.  Per block, after the post-rotation, each wave publishes its v (and
// its blksw) and one workgroup barrier later reads the other's.  Rows and v are double-buffered by block parity, so that
// one barrier per block suffices: a wave writes parity p again only after the next block's barrier, which the other wave
// passes only after it has read parity p.  The band energies of include/ac3mi.h: lane l < 53 takes the bins 13 + 4l ..
// 16 + 4l below 223 of both rows (the band edges 13, 25, 37, 61 are 13 + 4 x {0, 3, 6, 12}: no lane straddles one), four
// sums of squares as u64, split into 20-bit low and high parts that a 32-bit prefix scan sums exactly; the band totals
// are the scan at lanes 2, 5, 11 and 63.  Both waves compute the same flags.  A block with a flag rewrites each wave's
// own four bins (aligned, M or S) in registers before the exponents; the barrier is a bare s_barrier behind an LDS-only
// fence, so the next block's PCM loads (nxtv) stay in flight across it.
#ifndef ENC_MDCT_REMAT_LB
#define ENC_MDCT_REMAT_LB 5          // 90 VGPRs, no scratch (at 6: 80 VGPRs and 20 bytes of scratch, at 7: 72 and 52)
#endif
#ifndef ENC_MDCT_BSW_REMAT_LB
#define ENC_MDCT_BSW_REMAT_LB 4      // with block switching: 118 VGPRs, no scratch (at 5: 96 VGPRs and 48 bytes of scratch)
#endif
// BW (ac3mi_set_encode_bandwidth 1 or 2, with REMAT only - the other variants take P.x.nbc at run time already): the fourth
// rematrixing band ends at nbc = 73 + 3 chbwcod instead of 223.  nbc can split a lane's four bins only inside that band.
// XS (ac3mi_set_encode_exp_strategy 1): the exponent stage chooses the strategies by cost (exp_stage<false, 1>).
// LFEROW (2/0+LFE with rematrixing, never with BSW or REMAT): the plain kernel restricted to the LFE row, one wavefront per
// frame (unit = frame, channel nch - 1), launched beside the two-wavefront REMAT workgroups, which code channels 0 and 1.
// The LFE never switches: with block switching on it leaves its row's decision 0.
// FX (the plain kernel only; launch_encode's fixed-shape rule): one-frame 5.1 streams - six channels, the last the LFE, one
// frame, 223 coefficients, the history stored here and no tap, as constants: no division by nch or frames, strides of 6.
template <bool BSW, bool REMAT, bool BW = false, bool XS = false, bool LFEROW = false, bool FX = false>
__global__ __launch_bounds__(REMAT ? 128 : 64, REMAT ? (BSW ? ENC_MDCT_BSW_REMAT_LB : ENC_MDCT_REMAT_LB) : BSW ? ENC_MDCT_BSW_LB : ENC_MDCT_LB)
void enc_mdct_kernel(const MdctParams P)
{
    __shared__ int32_t out_[REMAT ? 4 : 1][256];        // REMAT: [2 * block parity + wave]
    __shared__ ExpLDS XL_[REMAT ? 2 : 1];
    __shared__ int rv_[REMAT ? 2 : 1][2];              // REMAT: [block parity][wave] = v | blksw << 8

    const int wave = REMAT ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0;
    const int lane = REMAT ? (int)(threadIdx.x & 63u) : (int)threadIdx.x;
    ExpLDS &XL = XL_[wave];
    // The nch wavefronts of a frame de-interleave the same PCM lines, one channel each.  Workgroups are dealt round-robin over the
    // 8 XCDs (private L2s), so with unit = blockIdx the channels of a frame sat on different XCDs and each fetched the frame's
    // samples for itself (PMC: 114 KB fetched per frame against 18 KB of PCM).  The bijective remap of cdna_hip_programming.md
    // (T1) makes consecutive units share an XCD: blocks with equal blockIdx % 8 take one contiguous range of units.  With
    // REMAT a unit is a workgroup = a stereo frame (the same bijection over gridDim.x = frames), its waves the channels.
    // (s*F + f)*nch + ch; REMAT: s*F + f.  Wave-uniform by construction: row and state addresses on the scalar unit
    const int unit = __builtin_amdgcn_readfirstlane((int)xcd_remap(blockIdx.x, gridDim.x));
    static_assert(!(LFEROW && (BSW || REMAT)), "the LFE row alone takes the plain kernel");
    static_assert(!(FX && (BSW || REMAT || BW || XS || LFEROW)), "the fixed 5.1 shape is the plain kernel's");
    const int nch = FX ? 6 : P.nch, frames = FX ? 1 : P.frames, nbc = FX ? 223 : P.x.nbc;
    const int ch = REMAT ? wave : LFEROW ? nch - 1 : unit % nch;
    const int sf = REMAT || LFEROW ? unit : unit / nch;
    const int f = sf % frames;
    const int s = sf / frames;

    // Which samples a lane owns.  Point i of the pre-rotation (:578-591) takes four samples of the 512 windowed ones:
    //   i < 64 :  re <- -in[384 + 2i], in[383 - 2i]     im <- in[128 + 2i], in[127 - 2i]
    //   i >= 64:  re <-  in[2i - 128], in[383 - 2i]     im <- in[128 + 2i], -in[639 - 2i]
    // so a lane that holds positions {2L, 127 - 2L, 128 + 2L, 255 - 2L} of the old AND of the new half has every operand of
    // the points L and L + 64 in its own registers; and with L = the lane number's six bits reversed those two points are
    // the ones the bit-reversed order (:496-504) puts at 2 lane and 2 lane + 1: its first butterfly.  Windowing, block floating
    // point, rotation and the reordering then need no LDS at all (same operands, same 16-bit truncations).
    const int L = (int)(__builtin_bitreverse32((unsigned)lane) >> 26);
    const int jpos[4] = {2 * L, 127 - 2 * L, 128 + 2 * L, 255 - 2 * L};
    int wa[4], wb[4];
#pragma unroll
    for (int k = 0; k < 4; k++) { wa[k] = P.tab->win[jpos[k]]; wb[k] = P.tab->win[255 - jpos[k]]; }
    static_assert(offsetof(EncTables, latab) % 4 == 0 && offsetof(EncTables, band_of_bin) % 4 == 0 && offsetof(MaskTabs, band_of_bin) % 4 == 0, "dword copies");
    reinterpret_cast<uint32_t *>(XL.t.latab)[lane] = reinterpret_cast<const uint32_t *>(P.tab->latab)[lane];
    reinterpret_cast<uint32_t *>(XL.t.band_of_bin)[lane] = reinterpret_cast<const uint32_t *>(P.tab->band_of_bin)[lane];
    if (lane < 50) XL.t.hth[lane] = P.tab->hth[lane][P.x.fscod];
    if (lane < 52) XL.t.band_start[lane] = lane < 51 ? P.tab->band_start[lane] : 0;
    // rotation factors of the points the lane rotates BEFORE the passes (L, L + 64) and AFTER them (lane, lane + 64; :596-602),
    // and the twiddles of its butterfly in passes 2..6 (:533-567: twiddle index (lane mod nloops) * nblocks): constant per lane
    int xcv[2], xsv[2], pcv[2], psv[2], twc[5], tws[5];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        xcv[k] = P.tab->xcos[lane + 64 * k]; xsv[k] = P.tab->xsin[lane + 64 * k];
        pcv[k] = -P.tab->xcos[L + 64 * k]; psv[k] = P.tab->xsin[L + 64 * k];
    }
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const int nloops = 4 << k, nblocks = 16 >> k, m = lane & (nloops - 1);
        // (a group's first butterfly, m == 0, takes no multiply in the reference: the twiddle that multiplies to the same - mdct_rule.h)
        const int tc = P.tab->cos[m * nblocks], ts = -P.tab->sin[m * nblocks];       // (loaded by every lane: selects, no exec regions)
        static_assert(MDCT_TW_ONE_IM == 0, "sin[0] is 0 already");
        twc[k] = m == 0 ? MDCT_TW_ONE_RE : tc;
        tws[k] = ts;
    }
    // the short pair: lane = 32 tsh + ls holds points Ls = bitrev5(ls) and Ls + 32 of transform tsh before the passes, ls and
    // ls + 32 after them (rotation factors read per switched block, from L1: held across the loop they spill)
    const int ls = lane & 31, Ls = (int)(__builtin_bitreverse32((unsigned)ls) >> 27), tsh = lane >> 5;
    const bool lfe = FX ? true : P.x.lfe != 0, lfe_ch = lfe && ch == nch - 1;

    const int16_t *frame_pcm = P.pcm + ((size_t)s * frames + f) * 1536 * nch + P.chmap[ch];
    // the lane's four samples of: the block before (history), this block, and - in flight while this block is
    // transformed - the next one.  Every sample is read from HBM once.
    int16_t oldv[4], newv[4], nxtv[4];
    int joff[4];                                    // the lane's positions as sample offsets (32-bit index arithmetic)
#pragma unroll
    for (int k = 0; k < 4; k++) joff[k] = __mul24(jpos[k], nch);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int j = jpos[k];
        if (f > 0) oldv[k] = frame_pcm[joff[k] - 256 * nch];                   // block 5 of the previous frame
        else oldv[k] = P.slot ? P.last[((size_t)P.slot[s] * 6 + ch) * 256 + j] : P.last[((size_t)s * nch + ch) * 256 + j];
        newv[k] = frame_pcm[joff[k]];
    }
    int rprev = 0;                                  // REMAT: the flags of the block before
    for (int blk = 0; blk < 6; blk++) {
        int32_t *const out = out_[REMAT ? 2 * (blk & 1) + wave : 0];
        int16_t *const zs = reinterpret_cast<int16_t *>(out);    // BSW: 512 16-bit samples staged in the coefficient row's LDS
        // ---- BSW: the transient detector (include/ac3mi.h) on the raw samples: z = old || new ----
        bool sw = false;
        if constexpr (BSW) {
#pragma unroll
            for (int k = 0; k < 4; k++) { zs[jpos[k]] = oldv[k]; zs[256 + jpos[k]] = newv[k]; }
            wave_sync();
            const int n0 = 8 * lane;
            int zm2 = lane ? zs[n0 - 2] : 0, zm1 = lane ? zs[n0 - 1] : 0, m = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int z = zs[n0 + j];
                const int y = z - 2 * zm1 + zm2;
                if (lane || j >= 2) m = max(m, y < 0 ? -y : y);
                zm2 = zm1; zm1 = z;
            }
            m = max(m, __shfl_xor(m, 1));
            m = max(m, __shfl_xor(m, 2));
            m = max(m, __shfl_xor(m, 4));
            int g[8];                                               // maxima of the 64-sample segments of [0, 512)
#pragma unroll
            for (int k = 0; k < 8; k++) g[k] = __builtin_amdgcn_readlane(m, 8 * k);
            const int p10 = max(max(g[0], g[1]), max(g[2], g[3])), p11 = max(max(g[4], g[5]), max(g[6], g[7]));
            const int p20 = max(g[2], g[3]), p21 = max(g[4], g[5]), p22 = max(g[6], g[7]);
            sw = !lfe_ch && p11 > 400 &&
                 (p11 > 10 * p10 || 3 * p21 > 40 * p20 || 3 * p22 > 40 * p21 ||
                  g[4] > 20 * g[3] || g[5] > 20 * g[4] || g[6] > 20 * g[5] || g[7] > 20 * g[6]);
            wave_sync();                                            // (every lane has read z before the row reuses the LDS)
        }
        // ---- 512 input samples: 256 old + 256 new (:1673-1683), windowed (:1686-1693) - in registers ----
        int win_[8];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int j = jpos[k];
            nxtv[k] = blk < 5 ? frame_pcm[(blk + 1) * 256 * nch + joff[k]] : (int16_t)0;
            if ((FX || P.store_history) && blk == 5) {
                if (P.slot) P.last[((size_t)P.slot[s] * 6 + ch) * 256 + j] = newv[k];
                else P.last[((size_t)s * nch + ch) * 256 + j] = newv[k];
            }
            // (a 16-bit sample times a window value in 0 .. 32767, >> 15, is a 16-bit value again: no truncation to restate)
            win_[k] = __mul24(oldv[k], wa[k]) >> 15;
            win_[4 + k] = __mul24(newv[k], wb[k]) >> 15;
            oldv[k] = newv[k];
        }
        // ---- block floating point (:1697-1700): v from the position of the largest magnitude's top bit (the reference ORs the
        //      magnitudes, :1570-1596; the maximum has the same top bit) ----
        const int acc = wave_max_nonneg(mdct_mag8(win_));
        int v = 14 - ilog2u((unsigned)acc);
        if (v < 0) v = 0;
        int shift = v - 9;
        int O[4], N[4];                                                     // in[jpos[k]], in[256 + jpos[k]] as 16-bit values
        // (|x| << v < 2^15 by the choice of v, or v = 0: the shifted values are 16-bit values already)
#pragma unroll
        for (int k = 0; k < 4; k++) { O[k] = win_[k] << v; N[k] = win_[4 + k] << v; }
        // ---- rotation + pre-rotation (:578-591) of the points L (-> p) and L + 64 (-> q) ----
        int pr, pi, qr, qi;
        if (BSW && sw) {
            // the short pair: point i of the lane's transform takes rot[2i], rot[255 - 2i], rot[128 + 2i], rot[127 - 2i] of its
            // 256 rotated samples - transform 1: rot = in[0..255]; transform 2: rot = -in[384..511] || in[256..383]
#pragma unroll
            for (int k = 0; k < 4; k++) { zs[jpos[k]] = (int16_t)O[k]; zs[256 + jpos[k]] = (int16_t)N[k]; }
            wave_sync();
            int rr[2], ri[2], spc[2], sps[2];
#pragma unroll
            for (int k = 0; k < 2; k++) { spc[k] = -P.tab->xcos2[Ls + 32 * k]; sps[k] = P.tab->xsin2[Ls + 32 * k]; }
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int i2 = 2 * (Ls + 32 * k), base = 256 * tsh;
                const int a = zs[base + (tsh ? 128 + i2 : i2)], b = zs[base + (tsh ? 127 - i2 : 255 - i2)];
                const int c = zs[base + (tsh ? i2 : 128 + i2)], d = zs[base + (tsh ? 255 - i2 : 127 - i2)];
                const int a2 = tsh ? (int)(int16_t)(-a) : a, d2 = tsh ? (int)(int16_t)(-d) : d;
                const int re = (a2 - b) >> 1, im = (-(c - d2)) >> 1;
                rr[k] = (int16_t)((__mul24(re, spc[k]) - __mul24(im, sps[k])) >> 15);
                ri[k] = (int16_t)((__mul24(re, sps[k]) + __mul24(spc[k], im)) >> 15);
            }
            pr = rr[0]; pi = ri[0]; qr = rr[1]; qi = ri[1];
            wave_sync();                                            // (z is read everywhere before the post-rotation writes the row)
        } else {
            const int re0 = ((int)(int16_t)(-N[2]) - N[1]) >> 1, im0 = (-(O[2] - O[1])) >> 1;
            const int re1 = (O[0] - O[3]) >> 1, im1 = (-(N[0] - (int)(int16_t)(-N[3]))) >> 1;
            // (every product of this kernel has operands of 17 bits at most: the 24-bit multiplier, not the quarter-rate 32-bit one)
            pr = (int16_t)((__mul24(re0, pcv[0]) - __mul24(im0, psv[0])) >> 15);
            pi = (int16_t)((__mul24(re0, psv[0]) + __mul24(pcv[0], im0)) >> 15);
            qr = (int16_t)((__mul24(re1, pcv[1]) - __mul24(im1, psv[1])) >> 15);
            qi = (int16_t)((__mul24(re1, psv[1]) + __mul24(pcv[1], im1)) >> 15);
        }
        // ---- the seven passes (:508-567) in registers: the lane's butterfly of pass k takes the points ip = (lane / d) 2d +
        //      lane mod d and ip + d (d = 2^k); between two passes every lane trades ONE point with lane ^ d (the upper half of
        //      a 2d-lane group gives its first point and keeps the second, the lower half the other way round).  Same operands,
        //      shifts and 16-bit truncations as the reference's in-place loops, no LDS round trip per pass. ----
        auto bfly_r = [&](int ax, int ay) {
            const int bx = pr, by = pi;
            pr = (int16_t)((bx + ax) >> 1);
            pi = (int16_t)((by + ay) >> 1);
            qr = (int16_t)((bx - ax) >> 1);
            qi = (int16_t)((by - ay) >> 1);
        };
        // lane ^ d without LDS: quad permutes (d = 1, 2), row shifts by bank (4), a row rotation (8); for d = 16 and 32 the trade
        // IS gfx950's v_permlane16_swap / v_permlane32_swap of (p, q): odd rows / the upper half of p against even rows / the
        // lower half of q
        auto trade = [&](auto dc) {
            constexpr int d = decltype(dc)::value;
            if constexpr (d == 32) {
                const auto r = __builtin_amdgcn_permlane32_swap((unsigned)pr, (unsigned)qr, false, false);
                const auto i = __builtin_amdgcn_permlane32_swap((unsigned)pi, (unsigned)qi, false, false);
                pr = (int)r[0]; qr = (int)r[1]; pi = (int)i[0]; qi = (int)i[1];
            } else if constexpr (d == 16) {
                const auto r = __builtin_amdgcn_permlane16_swap((unsigned)pr, (unsigned)qr, false, false);
                const auto i = __builtin_amdgcn_permlane16_swap((unsigned)pi, (unsigned)qi, false, false);
                pr = (int)r[0]; qr = (int)r[1]; pi = (int)i[0]; qi = (int)i[1];
            } else if constexpr (d == 4 || d == 8) {
                // the DPP bank mask does the selecting: the lower lanes' q takes the partner's p, the upper lanes' p the
                // partner's (old) q - four moves and two copies where selects around one move per component took eight to ten
                constexpr int lo_banks = d == 4 ? 0x5 : 0x3, up_banks = d == 4 ? 0xa : 0xc;
                constexpr int from_above = d == 4 ? 0x104 : 0x128, from_below = d == 4 ? 0x114 : 0x128;     // row_shl:4 / row_shr:4, row_ror:8
                const int qr0 = qr, qi0 = qi;
                qr = __builtin_amdgcn_update_dpp(qr, pr, from_above, 0xf, lo_banks, false);
                qi = __builtin_amdgcn_update_dpp(qi, pi, from_above, 0xf, lo_banks, false);
                pr = __builtin_amdgcn_update_dpp(pr, qr0, from_below, 0xf, up_banks, false);
                pi = __builtin_amdgcn_update_dpp(pi, qi0, from_below, 0xf, up_banks, false);
            } else {
                quad_trade2<d>(pr, pi, qr, qi);                              // one select through the quad permute per component
            }
        };
        bfly_r(qr, qi);                                                     // pass 0
        trade(std::integral_constant<int, 1>{});
        if (lane & 1) bfly_r(qi, -qr); else bfly_r(qr, qi);                 // pass 1: twiddles 1 and -j
        trade(std::integral_constant<int, 2>{});
        auto pass = [&](int k) {                                            // passes 2..6
            const int c = twc[k], sx = tws[k];
            const int tr = (__mul24(c, qr) - __mul24(sx, qi)) >> 15;
            const int ti = (__mul24(c, qi) + __mul24(qr, sx)) >> 15;
            bfly_r(tr, ti);
        };
        pass(0); trade(std::integral_constant<int, 4>{});
        pass(1); trade(std::integral_constant<int, 8>{});
        pass(2); trade(std::integral_constant<int, 16>{});
        pass(3);
        if (BSW && sw) {
            // the short pair's post-rotation: the lane holds points ls and ls + 32 of its transform; X[2i] = im, X[127 - 2i] = re,
            // interleaved into the row as coef[2k + transform]
            int sxc[2], sxs[2];
#pragma unroll
            for (int k = 0; k < 2; k++) { sxc[k] = P.tab->xcos2[ls + 32 * k]; sxs[k] = P.tab->xsin2[ls + 32 * k]; }
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int i = ls + 32 * k, zr = k ? qr : pr, zi = k ? qi : pi;
                out[4 * i + tsh] = (__mul24(zr, sxc[k]) + __mul24(sxs[k], zi)) >> 15;
                out[254 - 4 * i + tsh] = (__mul24(zr, sxs[k]) - __mul24(zi, sxc[k])) >> 15;
            }
        } else {
            trade(std::integral_constant<int, 32>{});
            pass(4);
            // ---- post-rotation (:596-602): the lane now holds points lane and lane + 64 ----
            {
                const int sx0 = xsv[0], c0 = xcv[0], sx1 = xsv[1], c1 = xcv[1];
                out[2 * lane] = (__mul24(pr, c0) + __mul24(sx0, pi)) >> 15;
                out[255 - 2 * lane] = (__mul24(pr, sx0) - __mul24(pi, c0)) >> 15;
                out[2 * (lane + 64)] = (__mul24(qr, c1) + __mul24(sx1, qi)) >> 15;
                out[255 - 2 * (lane + 64)] = (__mul24(qr, sx1) - __mul24(qi, c1)) >> 15;
            }
        }
        wave_sync();
        // ---- exponents (:1707-1722) ----
        const size_t row = (((size_t)s * frames + f) * 6 + blk) * nch + ch;
        int4 cv = *reinterpret_cast<const int4 *>(&out[4 * lane]);
        int cc[4] = {cv.x, cv.y, cv.z, cv.w};
        if constexpr (REMAT) {
            // ---- rematrixing (include/ac3mi.h): both rows, one barrier ----
            const int par = blk & 1;
            if (lane == 0) rv_[par][wave] = v | (sw ? 1 << 8 : 0);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
            const int r0 = rv_[par][0], r1 = rv_[par][1];
            const int vl = r0 & 0xff, vr = r1 & 0xff, vm = min(vl, vr), dl = vl - vm, dr = vr - vm;
            const int32_t *rl = out_[2 * par], *rr = out_[2 * par + 1];
            const int jend = BW ? nbc : 223;                    // the fourth band's end
            uint64_t el = 0, er = 0, em = 0, es = 0;
            if (lane < 53) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int j = 13 + 4 * lane + k;
                    if (j < jend) {
                        const int a = rl[j] >> dl, b = rr[j] >> dr, m = (a + b) >> 1, d = (a - b) >> 1;
                        el += (uint64_t)(uint32_t)abs(a) * (uint32_t)abs(a);
                        er += (uint64_t)(uint32_t)abs(b) * (uint32_t)abs(b);
                        em += (uint64_t)(uint32_t)abs(m) * (uint32_t)abs(m);
                        es += (uint64_t)(uint32_t)abs(d) * (uint32_t)abs(d);
                    }
                }
            }
            // (a lane's sums are below 2^36: 20-bit low parts and the high parts scan to below 2^26 and 2^22)
            const uint64_t e4[4] = {el, er, em, es};
            uint64_t eb[4][4];                                      // [quantity][band]
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t lo = wave_incl_scan_u32((uint32_t)e4[q] & 0xfffffu), hi = wave_incl_scan_u32((uint32_t)(e4[q] >> 20));
                const int at[4] = {2, 5, 11, 63};
                uint64_t prev = 0;
#pragma unroll
                for (int bd = 0; bd < 4; bd++) {
                    const uint64_t t = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)hi, at[bd]) << 20) +
                                       (uint32_t)__builtin_amdgcn_readlane((int)lo, at[bd]);
                    eb[q][bd] = t - prev;
                    prev = t;
                }
            }
            int flags = 0;
            if (!BSW || ((r0 ^ r1) & 0x100) == 0) {
#pragma unroll
                for (int bd = 0; bd < 4; bd++) {
                    const uint64_t ems = eb[2][bd] < eb[3][bd] ? eb[2][bd] : eb[3][bd];
                    const uint64_t elr = eb[0][bd] < eb[1][bd] ? eb[0][bd] : eb[1][bd];
                    if (2 * ems < elr) flags |= 1 << bd;
                }
            }
            if (flags) {
                // rows L' = cL >> dl, R' = cR >> dr at shift vm - 9; M / S in the flagged bands
                const int32_t *ro = wave ? rl : rr;
                const int dmine = wave ? dr : dl, doth = wave ? dl : dr;
                const int4 ov = *reinterpret_cast<const int4 *>(&ro[4 * lane]);
                const int oc[4] = {ov.x, ov.y, ov.z, ov.w};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int j = 4 * lane + k;
                    const int bd = j < 13 ? -1 : j < 25 ? 0 : j < 37 ? 1 : j < 61 ? 2 : j < jend ? 3 : -1;
                    const int a = cc[k] >> dmine, b = oc[k] >> doth;
                    cc[k] = bd >= 0 && ((flags >> bd) & 1) ? (wave ? (b - a) >> 1 : (a + b) >> 1) : a;
                }
                shift = vm - 9;
            }
            if (lane == 0 && wave == 0) P.remat[(size_t)sf * 6 + blk] = (uint8_t)(flags | (blk == 0 || flags != rprev ? 0x10 : 0));
            rprev = flags;
        }
        // (mdct_rule.h: no branch; the low bytes of the four exponents gathered by three byte permutes)
        int e4[4];
#pragma unroll
        for (int k = 0; k < 4; k++) e4[k] = mdct_raw_exp(cc[k], shift);
        const uint32_t epack = __builtin_amdgcn_perm(__builtin_amdgcn_perm((uint32_t)e4[3], (uint32_t)e4[2], 0x0c0c0400u),
                                                     __builtin_amdgcn_perm((uint32_t)e4[1], (uint32_t)e4[0], 0x0c0c0400u), 0x05040100u);
        // (the packers read a row's coded bins only: nbc of a full-bandwidth channel, 7 of the LFE - a quarter of the store traffic.
        //  Every reader of a row masks what lies beyond: the search and the packers give bins >= nbc exponent 255 (bap 0, no bits),
        //  enc_cpl_kernel reads [cplstrtmant, cplendmant) and, for a coupled channel's exponents, bins below cplstrtmant only)
        if ((!FX && P.full_rows) || 4 * lane < (lfe_ch ? 7 : nbc))
            *reinterpret_cast<int4 *>(P.mdct + row * 256 + 4 * lane) = make_int4(cc[0], cc[1], cc[2], cc[3]);
        if (!FX && P.expo) *reinterpret_cast<uint32_t *>(P.expo + row * 256 + 4 * lane) = epack;       // tap only
        *reinterpret_cast<uint32_t *>(&XL.E[blk][4 * lane]) = epack;
        if (lane == 0) P.shift[row] = (int8_t)shift;
        if constexpr (BSW) if (lane == 0) P.bsw[row] = sw ? 1 : 0;
        if constexpr (LFEROW) if (lane == 0 && P.bsw) P.bsw[row] = 0;
        (void)rprev;
#pragma unroll
        for (int k = 0; k < 4; k++) newv[k] = nxtv[k];
        wave_sync();
    }
    exp_stage<false, XS ? 1 : 0, FX>(P.x, XL, (size_t)sf, ch, lane);
}


// ---------------------------------------------------------------------------------------------
// enc_cpl_kernel: channel coupling (ac3mi_set_encode_coupling 1; the rule is include/ac3mi.h's).  One wavefront per frame,
// after enc_mdct_kernel, on the rows and exp_samples it left: per block the coupling row (the full-bandwidth rows aligned to
// the block's smallest exp_samples, summed over [cplstrtmant, 217), >> cpl_g(nfbw)), the exact band energies of the frame
// (u64 LDS atomics), the frame decision, the coordinates; then, for a coupled frame only, the coupling row's exponent stage
// (strategies as exp_stage's, exponents from cplstrtmant with 2 cplabsexp in front, masks from cplstrtbnd seeded with the
// coupling leaks) and the coupled channels' exponent stage again over [0, cplstrtmant) with their mode-0 strategies.  An
// uncoupled frame keeps everything enc_mdct_kernel wrote: its bytes are mode 0's.
struct CplParams {
    const int32_t *mdct;        // [S][F][6][nch][256]
    const int8_t *shift;        // [S][F][6][nch]
    const uint8_t *bsw;         // optional [S][F][6][nch]: a frame with a switched full-bandwidth block is not coupled
    uint8_t *remat;             // optional [S][F][6] (2/0, rematrixing on): rewritten for coupled frames; rows from w.prow
    int32_t *mdct_out;          // with remat: the coded rows of a coupled frame ([S][F][6][2][256])
    int8_t *shift_out;
    CplWs w;
    ExpParams x;                // the channels' exponent stage, x.nbc = cplstrtmant
    int nfbw, begf, nfr;
    int endf;                   // enc_cpl_kernel<true>: cplendf (begf <= endf + 2); <false>: 12
    int nbc;                    // enc_cpl_kernel<true>: the channels' nbc (rows are stored below it only); <false>: 223
};

struct CplLDS {
    ExpLDS X;
    uint8_t E1[6][256];                 // rematrixing: channel 1's raw exponents while X.E holds channel 0's
    unsigned long long rq[4][4];        // rematrixing: [L, R, M, S][band] sums of squares of one block
    unsigned long long en[6][16];       // [coupled channel, 5 = coupling row][band]: sums of squares over the frame
    unsigned long long score[5][4];     // [channel][mstrcplco]: sum over the bands of the coded coordinate squared
    int sh[6][8];                       // [block][channel]: exp_samples
};

__host__ __device__ constexpr int cpl_g(int nfbw) { return nfbw <= 2 ? 1 : nfbw <= 4 ? 2 : 3; }

// The coordinate of one channel and band under mstrcplco M (liba52 parse.c:642-656): the largest value mant 2^-s,
// E < 15: mant = 16 + m, s = E + 3M + 2;  E = 15: mant = m, s = 16 + 3M, with mant^2 Ecpl <= Ech (exact, 128-bit).
// Ech = 0 gives the zero coordinate (E 15, m 0) whatever Ecpl is: with Ecpl = 0 as well - a band of digital silence - every
// value fits, and the largest would play the decoder's dither of the coupling channel 7.75 times louder.
// Returns E << 4 | m, and mant, s.
__device__ __forceinline__ int cpl_quant(unsigned long long ech, unsigned long long ecpl, int M, int &mant, int &sv)
{
    if (ech == 0) {
        mant = 0; sv = 16 + 3 * M;
        return 15 << 4;
    }
    auto fits = [&](int mt, int s_) {
        return (unsigned __int128)(unsigned)(mt * mt) * ecpl <= ((unsigned __int128)ech << (2 * s_));
    };
    for (int E = 0; E < 15; E++) {
        const int s_ = E + 3 * M + 2;
        if (!fits(16, s_)) continue;
        int m = 15;
        while (!fits(16 + m, s_)) m--;
        mant = 16 + m; sv = s_;
        return E << 4 | m;
    }
    const int s_ = 16 + 3 * M;
    int m = 15;
    while (m > 0 && !fits(m, s_)) m--;
    mant = m; sv = s_;
    return 15 << 4 | m;
}

// The coupling row's exponents (encode_exp with the coupling start, cf. A/52 7.1.3): three entries a group from cs (the range
// is a multiple of 12 bins: no entry is left over) under the +-2 constraint (cpl_exp_entries, exp_constrain: enc_exp.h),
// written back to their bins; the reference exponent in front, 2 cplabsexp = entry 0 & ~1, goes to bin cs - 1.  Returns the
// bits of cplabsexp and the groups.
__device__ int cpl_encode_exp(uint8_t *row, int cs, int ce, int strategy, int lane)
{
    const int gs = syn_grpsize(strategy), groups = syn_cpl_exp_groups(cs, ce, strategy);
    int g[3], ix[3];
    bool valid[3];
    cpl_exp_entries(row, cs, 3 * groups, gs, lane, g, ix, valid);
    const int ref = exp_constrain<3, false>(g, ix, valid, 0, lane) & ~1;        // (the head is entry 0, whose index is 0)
#pragma unroll
    for (int c = 0; c < 3; c++)
        if (valid[c])
            for (int k = 0; k < gs; k++) row[cs + (3 * lane + c) * gs + k] = (uint8_t)g[c];
    if (lane == 0) row[cs - 1] = (uint8_t)ref;
    return 4 + 7 * groups;
}

// The coupling row's masking curve (A/52 7.2.2: the coupling channel's loop, no lowcomp), one lane per band: band PSDs of
// bins [cs, ce) (a band that starts below cs integrates from cs), the leaks seeded with (cplfleak << 8) + 768 and
// (cplsleak << 8) + 768 before band cplstrtbnd.  Bands outside the coupling range get 0.
__device__ void cpl_mask_wave(const MaskTabs &T, const uint8_t *row, int16_t *mask, int cs, int ce, int sdecay, int fdecay,
                              int sgain, int dbknee, int fgain, int halfrate, int lane)
{
    const int b = lane, bs = T.band_of_bin[cs], bend = T.band_of_bin[ce - 1] + 1;
    const bool live = b >= bs && b < bend;
    int psd = 0;
    if (live) {
        const int lo = T.band_start[b] > cs ? T.band_start[b] : cs;
        const int hi = T.band_start[b + 1] < ce ? T.band_start[b + 1] : ce;
        psd = 3072 - ((int)row[lo] << 7);
        for (int j = lo + 1; j < hi; j++) {
            const int pj = 3072 - ((int)row[j] << 7);
            int t = (psd > pj ? psd - pj : pj - psd) >> 1;
            t = t > 255 ? 255 : t;
            psd = (psd > pj ? psd : pj) + (int)T.latab[t];
        }
    }
    int fast, slow;
    mask_leaks(psd, live, b, sdecay, fdecay, sgain, fgain, fast, slow);
    const int f0 = (CPL_FLEAK << 8) + 768 - (b - bs + 1) * fdecay, s0 = (CPL_SLEAK << 8) + 768 - (b - bs + 1) * sdecay;
    fast = fast > f0 ? fast : f0;
    slow = slow > s0 ? slow : s0;
    mask_store(T, mask, b, live, (int16_t)(fast > slow ? fast : slow), psd, dbknee, halfrate);
}

// BW (ac3mi_set_encode_bandwidth 1 or 2): the coupling range ends at cplendmant = 73 + 12 P.endf, 3 + endf - begf bands.
// XS (ac3mi_set_encode_exp_strategy 1): xs_choose picks the coupling row's strategies (its candidate rows through L.E1[0],
// free until the rematrixing part) and the coupled channels' over [0, cplstrtmant) (exp_stage<false, 2>).
// R3 (2/0+LFE with rematrixing): the rows before rematrixing (w.prow ...) and the coded rows have three rows a block, the
// LFE's last, which this kernel neither reads nor writes (enc_mdct_kernel<.., LFEROW> codes it); <false>: two (2/0)
template <bool BW = false, bool XS = false, bool R3 = false>
__global__ __launch_bounds__(64) void enc_cpl_kernel(const CplParams P)
{
    constexpr int RN = R3 ? 3 : 2;                      // rows a block of the rematrixing arrays (= nch when they are used)
    __shared__ CplLDS L;
    const int lane = threadIdx.x;
    const size_t fidx = blockIdx.x;
    const int nch = P.x.nch, nfbw = P.nfbw, g = cpl_g(nfbw);
    const int cs = 37 + 12 * P.begf, ce = BW ? 73 + 12 * P.endf : 217, nb = BW ? 3 + P.endf - P.begf : 15 - P.begf;
    const EncTables *tab = P.x.tab;
    ExpLDS &X = L.X;
    reinterpret_cast<uint32_t *>(X.t.latab)[lane] = reinterpret_cast<const uint32_t *>(tab->latab)[lane];
    reinterpret_cast<uint32_t *>(X.t.band_of_bin)[lane] = reinterpret_cast<const uint32_t *>(tab->band_of_bin)[lane];
    if (lane < 50) X.t.hth[lane] = tab->hth[lane][P.x.fscod];
    if (lane < 52) X.t.band_start[lane] = lane < 51 ? tab->band_start[lane] : 0;
    for (int i = lane; i < 6 * 16; i += 64) (&L.en[0][0])[i] = 0;
    if (lane < 20) (&L.score[0][0])[lane] = 0;
    const bool rm = P.remat != nullptr;                 // 2/0 with rematrixing: the rows before it (w.prow)
    if (lane < 6 * nch) L.sh[lane / nch][lane % nch] = rm ? P.w.pshift[fidx * (6 * RN) + lane] : P.shift[fidx * 6 * nch + lane];
    bool decline = false;
    if (P.bsw) decline = __ballot(lane < 6 * nch && lane % nch < nfbw && P.bsw[fidx * 6 * nch + lane] != 0) != 0;
    wave_sync();
    int fmin = 127;
    for (int b = 0; b < 6; b++)
        for (int ch = 0; ch < nfbw; ch++) fmin = L.sh[b][ch] < fmin ? L.sh[b][ch] : fmin;

    // ---- per block: the coupling row, its raw exponents, the energies ----
    const int32_t *md = rm ? P.w.prow + fidx * 6 * RN * 256 : P.mdct + fidx * 6 * nch * 256;
    for (int b = 0; b < 6; b++) {
        int shb = 127;
        for (int ch = 0; ch < nfbw; ch++) shb = L.sh[b][ch] < shb ? L.sh[b][ch] : shb;
        int S[4] = {0, 0, 0, 0};
#pragma unroll 1
        for (int ch = 0; ch < nfbw; ch++) {
            const int sc = L.sh[b][ch];
            const int4 cv = *reinterpret_cast<const int4 *>(md + (b * nch + ch) * 256 + 4 * lane);
            const int c4[4] = {cv.x, cv.y, cv.z, cv.w};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int j = 4 * lane + k;
                if (j >= cs && j < ce) {
                    S[k] += c4[k] >> (sc - shb);
                    const int a = c4[k] >> (sc - fmin);
                    atomicAdd(&L.en[ch][(j - cs) / 12], (unsigned long long)((long long)a * a));
                }
            }
        }
        int cr[4];
        uint32_t epack = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int j = 4 * lane + k;
            int v = j >= cs && j < ce ? S[k] >> g : 0;
            const int a = v < 0 ? -v : v;
            int e = 24;
            if (a) {
                e = 23 - ilog2u((unsigned)a) + shb;
                if (e >= 24) { e = 24; v = 0; }
            }
            cr[k] = v;
            epack |= (uint32_t)e << (8 * k);
            if (v) { const int q = v >> (shb - fmin); atomicAdd(&L.en[5][(j - cs) / 12], (unsigned long long)((long long)q * q)); }
        }
        *reinterpret_cast<int4 *>(P.w.mdct + (fidx * 6 + b) * 256 + 4 * lane) = make_int4(cr[0], cr[1], cr[2], cr[3]);
        *reinterpret_cast<uint32_t *>(&X.E[b][4 * lane]) = epack;
        if (lane == 0) P.w.shift[fidx * 8 + b] = (int8_t)shb;
    }
    wave_sync();

    // ---- the frame decision: no band where 4 E(sum) < sum of the channels' E, E(sum) = 2^(2 g) E(coupling row) ----
    {
        unsigned long long tot = 0;
        if (lane < nb)
            for (int ch = 0; ch < nfbw; ch++) tot += L.en[ch][lane];
        decline = decline || __ballot(lane < nb && (L.en[5][lane < nb ? lane : 0] << (2 * g + 2)) < tot) != 0;
    }
    if (decline) {
        if (lane == 0) P.w.word[fidx] = 0;
        return;
    }

    // ---- coordinates: per channel and band, for every mstrcplco; the channel's mstrcplco maximises the sum over its bands of
    //      the coded coordinate squared (ties: the smaller) ----
    int code[2][4];
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const int i = lane + 64 * r;
        if (i < nfbw * nb) {
            const int ch = i / nb, bd = i - ch * nb;
#pragma unroll
            for (int M = 0; M < 4; M++) {
                int mant, sv;
                code[r][M] = cpl_quant(L.en[ch][bd], L.en[5][bd], M, mant, sv);
                atomicAdd(&L.score[ch][M], (unsigned long long)(mant * mant) << (50 - 2 * sv));
            }
        }
    }
    wave_sync();
    uint32_t word = 1;
    for (int ch = 0; ch < nfbw; ch++) {
        int best = 0;
        for (int M = 1; M < 4; M++) best = L.score[ch][M] > L.score[ch][best] ? M : best;
        word |= (uint32_t)best << (8 + 2 * ch);
    }
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const int i = lane + 64 * r;
        if (i < nfbw * nb) {
            const int ch = i / nb, bd = i - ch * nb, M = (word >> (8 + 2 * ch)) & 3;
            const int cd = M == 0 ? code[r][0] : M == 1 ? code[r][1] : M == 2 ? code[r][2] : code[r][3];
            P.w.co[fidx * 80 + ch * 16 + bd] = (uint8_t)cd;
        }
    }
    if (lane == 0) P.w.word[fidx] = word;

    // ---- the coupling row's exponent stage ----
    {
        uint32_t raw[6];
#pragma unroll
        for (int b = 0; b < 6; b++) raw[b] = *reinterpret_cast<const uint32_t *>(&X.E[b][4 * lane]);
        int st[6];
        st[0] = 1;
        if constexpr (XS) {
            uint32_t in = 0;
#pragma unroll
            for (int c = 0; c < 4; c++) in |= (4 * lane + c >= cs && 4 * lane + c < ce ? 0xffu : 0u) << (8 * c);
            const uint32_t x = xs_choose<true>(X.E, L.E1[0], in, 0, cs, ce, 0, false, lane);
#pragma unroll
            for (int b = 0; b < 6; b++) st[b] = (int)((x >> (4 * b)) & 15u);
        } else {
            const uint32_t d1 = __builtin_amdgcn_sad_u8(raw[1], raw[0], 0u), d2 = __builtin_amdgcn_sad_u8(raw[2], raw[1], 0u);
            const uint32_t d3 = __builtin_amdgcn_sad_u8(raw[3], raw[2], 0u), d4 = __builtin_amdgcn_sad_u8(raw[4], raw[3], 0u);
            const uint32_t d5 = __builtin_amdgcn_sad_u8(raw[5], raw[4], 0u);
            const uint32_t t12 = wave_sum_u32(d1 | d2 << 16), t34 = wave_sum_u32(d3 | d4 << 16), t5 = wave_sum_u32(d5);
            st[1] = (t12 & 0xffffu) > 1000u; st[2] = (t12 >> 16) > 1000u;
            st[3] = (t34 & 0xffffu) > 1000u; st[4] = (t34 >> 16) > 1000u;
            st[5] = t5 > 1000u;
        }
        uint32_t starts = 0;
#pragma unroll
        for (int b = 0; b < 6; b++) starts |= (st[b] != 0 ? 1u : 0u) << b;
#pragma unroll
        for (int b = 0; b < 6; b++) {
            if (XS || st[b] == 0) continue;
            int run = 1;
#pragma unroll
            for (int e = 1; e < 6; e++) if (b + e < 6 && run == e && st[b + e] == 0) run = e + 1;
            st[b] = run == 1 ? 3 : run <= 3 ? 2 : 1;
        }
        uint32_t inside = 0;
#pragma unroll
        for (int c = 0; c < 4; c++) inside |= (4 * lane + c >= cs && 4 * lane + c < ce ? 0xffu : 0u) << (8 * c);
#pragma unroll
        for (int b = 0; b < 5; b++) {
            if (!((starts >> b) & 1u)) continue;
            bool open = true, touched = false;
#pragma unroll
            for (int e = b + 1; e < 6; e++) {
                open = open && !((starts >> e) & 1u);
                if (open) { raw[b] = bytes_min_where(raw[b], raw[e], inside); touched = true; }
            }
            if (touched) *reinterpret_cast<uint32_t *>(&X.E[b][4 * lane]) = raw[b];
        }
        wave_sync();
        int bits = 0;
        for (uint32_t m = starts; m; m &= m - 1) {
            const int b = __builtin_ctz(m);
            bits += cpl_encode_exp(X.E[b], cs, ce, st[b], lane);
        }
        wave_sync();
        constexpr int sdecaycod = 2, fdecaycod = 1, fgaincod = 4, sgaincod = 1, dbkneecod = 2;
        const int sdecay = enc_sdecay(sdecaycod) >> P.x.halfrate, fdecay = enc_fdecay(fdecaycod) >> P.x.halfrate;
        for (uint32_t m = starts; m; m &= m - 1) {
            const int b = __builtin_ctz(m);
            cpl_mask_wave(X.t, X.E[b], X.mask[b], cs, ce, sdecay, fdecay, enc_sgain(sgaincod), enc_dbknee(dbkneecod),
                          enc_fgain(fgaincod), P.x.halfrate, lane);
        }
        wave_sync();
        int src = 0;
        for (int b = 0; b < 6; b++) {
            src = ((starts >> b) & 1u) ? b : src;
            *reinterpret_cast<uint32_t *>(P.w.eexp + (fidx * 6 + b) * 256 + 4 * lane) = *reinterpret_cast<const uint32_t *>(&X.E[src][4 * lane]);
            if (lane < 50) P.w.emask[(fidx * 6 + b) * 50 + lane] = (int16_t)(X.mask[src][lane] - enc_floor(4));
        }
        if (lane < 6) P.w.strat[fidx * 8 + lane] = (uint8_t)(lane == 0 ? st[0] : lane == 1 ? st[1] : lane == 2 ? st[2] : lane == 3 ? st[3] : lane == 4 ? st[4] : st[5]);
        if (lane == 0) P.w.ebits[fidx] = bits;
        wave_sync();
    }

    if (rm) {
        // ---- 2/0 with rematrixing: the mode-1 rule again, over liba52's cplinu-1 bands (the last ends at cplstrtmant); the
        //      coded rows, their exp_samples and exponents (strategies from them, as enc_mdct_kernel<*, true> does) ----
        const int nrem = P.begf == 0 ? 2 : P.begf <= 2 ? 3 : 4;
        auto band_of = [&](int j) { return j < 13 || j >= cs ? -1 : j < 25 ? 0 : j < 37 ? 1 : j < 61 ? 2 : 3; };
        int prev = 0;
        for (int b = 0; b < 6; b++) {
            if (lane < 16) (&L.rq[0][0])[lane] = 0;
            wave_sync();
            const int vl = L.sh[b][0], vr = L.sh[b][1], vm = vl < vr ? vl : vr;
            const int4 lv = *reinterpret_cast<const int4 *>(md + (b * RN) * 256 + 4 * lane);
            const int4 rv = *reinterpret_cast<const int4 *>(md + (b * RN + 1) * 256 + 4 * lane);
            const int lc[4] = {lv.x, lv.y, lv.z, lv.w}, rc[4] = {rv.x, rv.y, rv.z, rv.w};
            int a[4], c[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                a[k] = lc[k] >> (vl - vm);
                c[k] = rc[k] >> (vr - vm);
                const int bd = band_of(4 * lane + k);
                if (bd >= 0) {
                    const long long m = (a[k] + c[k]) >> 1, d = (a[k] - c[k]) >> 1;
                    atomicAdd(&L.rq[0][bd], (unsigned long long)((long long)a[k] * a[k]));
                    atomicAdd(&L.rq[1][bd], (unsigned long long)((long long)c[k] * c[k]));
                    atomicAdd(&L.rq[2][bd], (unsigned long long)(m * m));
                    atomicAdd(&L.rq[3][bd], (unsigned long long)(d * d));
                }
            }
            wave_sync();
            int flags = 0;
            if (!P.bsw || P.bsw[(fidx * 6 + b) * RN] == P.bsw[(fidx * 6 + b) * RN + 1])
                for (int bd = 0; bd < nrem; bd++) {
                    const unsigned long long ems = L.rq[2][bd] < L.rq[3][bd] ? L.rq[2][bd] : L.rq[3][bd];
                    const unsigned long long elr = L.rq[0][bd] < L.rq[1][bd] ? L.rq[0][bd] : L.rq[1][bd];
                    if (2 * ems < elr) flags |= 1 << bd;
                }
            uint32_t ep[2] = {0, 0};
            int out[2][4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int bd = band_of(4 * lane + k);
                int x0 = flags ? a[k] : lc[k], x1 = flags ? c[k] : rc[k];
                if (bd >= 0 && ((flags >> bd) & 1)) { x0 = (a[k] + c[k]) >> 1; x1 = (a[k] - c[k]) >> 1; }
                const int xs[2] = {x0, x1};
#pragma unroll
                for (int ch = 0; ch < 2; ch++) {
                    const int sh = flags ? vm : L.sh[b][ch];
                    int x = xs[ch];
                    const int ax = x < 0 ? -x : x;
                    int e = 24;
                    if (ax) {
                        e = 23 - ilog2u((unsigned)ax) + sh;
                        if (e >= 24) { e = 24; x = 0; }
                    }
                    out[ch][k] = x;
                    ep[ch] |= (uint32_t)(e & 0xff) << (8 * k);
                }
            }
#pragma unroll
            for (int ch = 0; ch < 2; ch++) {
                const size_t row = (fidx * 6 + b) * RN + ch;
                *reinterpret_cast<int4 *>(P.mdct_out + row * 256 + 4 * lane) = make_int4(out[ch][0], out[ch][1], out[ch][2], out[ch][3]);
                if (lane == 0) P.shift_out[row] = (int8_t)(flags ? vm : L.sh[b][ch]);
            }
            *reinterpret_cast<uint32_t *>(&X.E[b][4 * lane]) = ep[0];
            *reinterpret_cast<uint32_t *>(&L.E1[b][4 * lane]) = ep[1];
            if (lane == 0) P.remat[fidx * 6 + b] = (uint8_t)(flags | (b == 0 || flags != prev ? 0x10 : 0));
            prev = flags;
        }
        wave_sync();
        exp_stage<false, XS ? 2 : 0>(P.x, X, fidx, 0, lane);
        wave_sync();
#pragma unroll
        for (int b = 0; b < 6; b++) *reinterpret_cast<uint32_t *>(&X.E[b][4 * lane]) = *reinterpret_cast<const uint32_t *>(&L.E1[b][4 * lane]);
        wave_sync();
        exp_stage<false, XS ? 2 : 0>(P.x, X, fidx, 1, lane);
        return;
    }

    // ---- the coupled channels' exponent stage over [0, cplstrtmant), with their mode-0 strategies ----
    for (int ch = 0; ch < nfbw; ch++) {
        for (int b = 0; b < 6; b++) {
            const int shc = L.sh[b][ch];
            const int4 cv = *reinterpret_cast<const int4 *>(md + (b * nch + ch) * 256 + 4 * lane);
            const int c4[4] = {cv.x, cv.y, cv.z, cv.w};
            uint32_t epack = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int a = c4[k] < 0 ? -c4[k] : c4[k];
                // (bins from nbc on: exponent 24 - the row store leaves them unwritten, so the exponent tap stays reproducible)
                const int e = 4 * lane + k >= (BW ? P.nbc : 223) || a == 0 ? 24 : 23 - ilog2u((unsigned)a) + shc;
                epack |= (uint32_t)(e & 0xff) << (8 * k);
            }
            *reinterpret_cast<uint32_t *>(&X.E[b][4 * lane]) = epack;
        }
        wave_sync();
        exp_stage<!XS, XS ? 2 : 0>(P.x, X, fidx, ch, lane);
        wave_sync();
    }
}


// bap of one coefficient for SNR offset `snroffset` (:393-420):
//   v = ((max(mask - snroffset - floor, 0)) & 0x1fe0) + floor,  address = (psd - v) >> 5,  psd = 3072 - 128 exp
//   =>  address = clamp(80 - 4 exp - max(0, (mask - floor - snroffset) >> 5), 0, 63)       (floor = 0x1f0)
// The search kernel works on 4 x address (a byte offset into bitlut): clamp(term - 16 exp, 0, 252) with the band's
// term = 320 - max(0, ((mask - floor - snroffset) >> 3) & ~3) (SearchLDS::terms); the packers on the address itself (enc_mant.h).
// L.bitlut[address] = plain mantissa width | (bap==1) << 9 | (bap==2) << 14 | (bap==4) << 19: 24 bits, so that a lane's sums
// over a frame's rows (width <= 6 x 4 x 16 = 384, counts <= 24) stay clear of each other and a sum can be added to a block's
// account with one v_mad_u32_u24.
typedef short pk2 __attribute__((ext_vector_type(2)));

// plain (ungrouped) mantissa width of a bap code; 0 for the grouped codes 1, 2, 4 and for 0
__device__ __forceinline__ int plain_bits(int bp)
{
    return bp == 3 ? 3 : bp == 5 ? 4 : bp == 14 ? 14 : bp == 15 ? 16 : bp >= 6 ? bp - 1 : 0;
}

// The reference's SNR-offset search (:921-967) as a resumable state machine: next() skips the steps that
// need no evaluation and names the next (csnroffst, fsnroffst) to try, consume() takes the verdict.
struct SnrSearch {
    int csnr, fsnr, phase;
    bool failed;
    __device__ __forceinline__ bool next(int &cc, int &ff)
    {
        for (;;) {
            cc = csnr; ff = fsnr;
            if (phase == 0) { if (csnr < 0) { failed = true; phase = 5; return false; } return true; }
            if (phase == 1) { if (csnr + 4 > 63) { phase = 2; continue; } cc = csnr + 4; return true; }
            if (phase == 2) { if (csnr + 1 > 63) { phase = 3; continue; } cc = csnr + 1; return true; }
            if (phase == 3) { if (fsnr + 4 > 15) { phase = 4; continue; } ff = fsnr + 4; return true; }
            if (phase == 4) { if (fsnr + 1 > 15) { phase = 5; return false; } ff = fsnr + 1; return true; }
            return false;
        }
    }
    __device__ __forceinline__ void consume(bool ok)
    {
        if (phase == 0) { if (ok) phase = 1; else csnr -= 4; }
        else if (phase == 1) { if (ok) csnr += 4; else phase = 2; }
        else if (phase == 2) { if (ok) csnr += 1; else phase = 3; }
        else if (phase == 3) { if (ok) fsnr += 4; else phase = 4; }
        else if (phase == 4) { if (ok) fsnr += 1; else phase = 5; }
    }
};

// Both CRC words of the staged frame (MSB-first dwords in LDS) by the lane rule of crc_lanes.h, on one whole wavefront:
// crc1 in the low half, crc2 in the high half, wave-uniform.  The lane's row is requested first and travels during the byte
// loop; nothing of it is live before this point.
template <class LDS>
__device__ __forceinline__ uint32_t frame_crcs(const LDS &L, const uint32_t *fr, const PackParams &P, int fs, int lane)
{
    const uint4 *row = reinterpret_cast<const uint4 *>(P.crc_rows) + 2 * lane;
    const uint4 r0 = row[0], r1 = row[1];
    const CrcSplit sp{P.crc_c, P.crc_n1};
    const CrcLane ln = crcl_lane(sp, fs, lane);
    const uint32_t sum = crcl_chunk_sum(fr, L.crc_tab, ln.begin, sp.C, ln.lo);
    const uint32_t r[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
    const uint32_t scan = wave_incl_scan_xor_u32(crcl_mul_row(sum, r));
    const uint32_t crc1 = (uint32_t)__builtin_amdgcn_readlane((int)scan, sp.n1 - 1);
    return crc1 | ((wave_last(scan) ^ crc1) << 16);
}

// PART 0: one wavefront per stream does everything, frames in order.
// PART 3 + PART 1 + PART 2: for few, long streams.  Only the search carries something from frame to frame (it starts
// from the previous frame's csnroffst).  PART 3 (one wavefront per frame) tabulates the fit verdicts around every
// frame's own optimum; PART 1 (one wavefront per stream) replays the reference's search sequence frame after frame
// from those tables - costing an offset itself only when the table has no answer - and leaves csnroffst / fsnroffst
// of every frame in P.snr; PART 2 (one wavefront per frame) packs all frames at once.
// Measurement aid (make EXTRA=-DPACK_STAMPS, a separate library): lane 0 of every wavefront adds the s_memtime cycles it
// spent in each section of a frame to g_pack_cycles: search kernel: 0 frame set-up + SNR-offset search, 4 = calls of
// cost_and_record, 5 = frames; enc_packf_kernel: 6 set-up, 1 header / side information / exponent groups, 2 mantissas, 3 CRCs +
// store, 7 = frames.  ac3mi_debug_pack_cycles reads them.
#ifdef PACK_STAMPS
__device__ unsigned long long g_pack_cycles[16];
#define PK_DECL() unsigned long long pk_t = 0, pk_acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}
#define PK_T0() pk_t = __builtin_readcyclecounter()
#define PK_LAP(id) do { const unsigned long long t_ = __builtin_readcyclecounter(); pk_acc[id] += t_ - pk_t; pk_t = t_; } while (0)
#define PK_COUNT(id) pk_acc[id] += 1
#define PK_END() do { if (lane == 0) for (int i_ = 0; i_ < 9; i_++) atomicAdd(&g_pack_cycles[i_], pk_acc[i_]); } while (0)
#else
#define PK_DECL() do { } while (0)
#define PK_T0() do { } while (0)
#define PK_LAP(id) do { } while (0)
#define PK_COUNT(id) do { } while (0)
#define PK_END() do { } while (0)
#endif

// offsets costed per sweep of the SNR-offset search (two per packed 16-bit pipeline).  4 saves a sweep now and then but costs
// registers and reductions: 6.01 - 6.04 against 5.92 ms per 65 536 one-frame streams, 1 % ahead on long streams; 3 stays
#ifndef ENC_NC
#define ENC_NC 3
#endif

#ifndef ENC_SEARCH_LB
#define ENC_SEARCH_LB 4          // 128 VGPRs; a fifth wavefront per SIMD (96 VGPRs, 28 bytes of scratch) measured the same 1.02 ms
#endif
// enc_search_kernel<1>: one wavefront per stream, frames in order; <3>: one wavefront per frame tabulates (see above).
// CPL (enc_search_cpl_kernel: channel coupling on, P.cpl): the coupling rows join the costed rows of a coupled frame.
// BW (with CPL; ac3mi_set_encode_bandwidth 1 or 2): a coupled frame ends at cplendmant = 73 + 12 P.cpl_endf, not 217.
// DRC (ac3mi_set_encode_drc 1..5): every block that sends a dynrng word (P.drc) costs its 8 bits.
// DW (with DRC; P.dyn / P.compr): the words of the caller's or the source's arrays instead - 8 bits per word a programme sends
// (dyn_sends) and per compr word; P.drc may then be null (no profile).
// FX (PART 1 with none of the above; launch_encode's fixed-shape rule): one-frame 5.1 streams - six channels, five of them
// full-bandwidth, acmod 7, 223 coefficients, a single frame and neither taps nor a verdict table, as constants instead of P's members.
template <int PART, bool CPL = false, bool BW = false, bool DRC = false, bool FX = false, bool DW = false>
__global__ __launch_bounds__(64, FX ? 7 : ENC_SEARCH_LB) void enc_search_kernel(const PackParams P)      // (FX: profiles/search_window_resources.md)
{
    static_assert(PART == 1 || PART == 3, "the packers are enc_packf_kernel / enc_packb_kernel");
    static_assert(!DW || DRC, "the array words are costed where the profiles' are");
    static_assert(!FX || (PART == 1 && !CPL && !BW && !DRC), "the fixed 5.1 shape is the plain per-stream search's");
    // The two sweeps live here.  WIN (PART 1, every instantiation): cost_window - one pass costs the sixteen offsets lo .. lo + 15
    // (snr_window.h).  PART 3 tabulates csnroffst values, offsets 16 apart, which no window holds two of: it keeps the
    // three-offset sweep cost_and_record, with ENC_NC and the probe policy around it.
    constexpr bool WIN = PART == 1;
    __shared__ SearchLDS<CPL, WIN> L;
    const int lane = threadIdx.x;
    constexpr bool PER_FRAME = PART == 3;
    const int s = PER_FRAME ? (int)(blockIdx.x / (unsigned)P.frames_per_stream) : (int)blockIdx.x;
    const int f_first = PER_FRAME ? (int)(blockIdx.x - (unsigned)s * (unsigned)P.frames_per_stream) : 0;
    const int f_end = PER_FRAME ? f_first + 1 : FX ? 1 : P.frames_per_stream;
    if (s >= P.n_streams) return;

    for (int i = lane; i < 256; i += 64) L.band_of_bin[i] = P.tab->band_of_bin[i];
    {
        const int bp = P.tab->baptab[lane];
        L.bitlut[lane] = (uint32_t)plain_bits(bp) | ((bp == 1) << 9) | ((bp == 2) << 14) | ((bp == 4) << 19);
    }
    // (window sweep) lane = band: the band's bins [band_lo, band_hi) as indices into L.scan
    int band_lo = 0, band_hi = 0;
    if constexpr (WIN) {
        const int b = lane < 50 ? lane : 49;
        band_lo = 3 + P.tab->band_start[b];
        band_hi = 3 + (b < 49 ? P.tab->band_start[b + 1] : 256);      // (band_of_bin: the last band holds every bin to 255)
        if (lane == 0) L.scan[3] = 0;
    }

    const int nch = FX ? 6 : P.nch, nfbw = FX ? 5 : P.nfbw, nbc = FX ? 223 : P.nbc;
    const int acmod = FX ? 7 : P.acmod;
    const bool lfe = FX ? true : P.lfe != 0;
    const int fs = P.frame_words;

    const int sslot = P.slot ? P.slot[s] : s;
    const int cpl_cs = 37 + 12 * P.cpl_begf;        // (coupling only)
    const int cpl_ce = BW ? 73 + 12 * P.cpl_endf : 217, cpl_nb = BW ? 3 + P.cpl_endf - P.cpl_begf : 15 - P.cpl_begf;
    // the stream's search state: csnroffst in bits 0-7, the fsnroffst of its last coded frame in bits 8-11 (what the
    // reference's s->csnroffst / s->fsnroffst[] hold between frames, ENC/ac3enc.cpp:969-972)
    const int state_in = P.csnr_state[sslot];
    int csnr_prev = state_in & 0xff, fsnr_prev = (state_in >> 8) & 15;
    PK_DECL();

    for (int f = f_first; f < f_end; f++) {
        const size_t fidx = FX ? (size_t)s : (size_t)s * P.frames_per_stream + f;
        PK_T0();
        PK_COUNT(5);
        const uint8_t *ex = P.eexp + fidx * 6 * nch * 256;
        int frame_bits = 0;
        uint64_t run_starts = 0, row_set = 0;
        int ncplrows = 0;                                           // coupling run-start rows behind the channels' in rowdesc
        const bool cplf = CPL && (__builtin_amdgcn_readfirstlane((int)P.cpl.word[fidx]) & 1);
        const uint8_t *cex = cplf ? P.cpl.eexp + fidx * 6 * 256 : ex;
        bool loaded = false;
        auto load_frame = [&]() {
            loaded = true;
        // ---- masking curves, strategies and exponent bit counts from exp_stage (the encoded exponents
            //      stay in HBM/L2: [blk][ch][256] bytes at `ex`; the window sweep leaves the masks there too) ----
            if constexpr (!WIN) {
                const uint32_t *gm = reinterpret_cast<const uint32_t *>(P.emask + fidx * 6 * nch * 50);
                uint32_t mv[15];
#pragma unroll
                for (int j = 0; j < 15; j++) {
                    const int i = lane + 64 * j;
                    mv[j] = i < 6 * nch * 25 ? gm[i] : 0;
                }
#pragma unroll
                for (int j = 0; j < 15; j++) {
                    const int i = lane + 64 * j;
                    if (i < 6 * nch * 25) reinterpret_cast<uint32_t *>(&L.mask[0][0])[i] = mv[j];
                }
            }
            if (lane < 6 * nch) { const int b = lane / nch, ch = lane - b * nch; L.strat[b][ch] = P.strat[fidx * 6 * nch + lane]; }
            frame_bits = wave_sum(lane < nch ? P.ebits[fidx * nch + lane] : 0);
            wave_sync();
            // rows (blk * 6 + ch) that send new exponents, i.e. start a run, as a bit set; and the same as bit 8*ch + b
            {
                const int b6 = lane / 6, c6 = lane - 6 * b6;
                row_set = __ballot(lane < 36 && c6 < nch && L.strat[lane < 36 ? b6 : 0][c6] != 0);
                const int c8 = lane >> 3, b8 = lane & 7;
                run_starts = __ballot(b8 < 6 && c8 < nch && L.strat[b8 < 6 ? b8 : 0][c8 < 6 ? c8 : 0] != 0);
                // one descriptor per run-start row, computed by the row's lane, compacted in row order: the sweeps then
                // walk a list instead of deriving block range, channel and addresses from bit sets (scalar work per row
                // and sweep: the scalar unit is what bounds the search)
                if (lane < 36 && ((row_set >> lane) & 1)) {
                    const uint32_t later = (uint32_t)((run_starts >> (8 * c6)) & 0x3f) | 0x40u;       // bit b: block b of this channel sends exponents
                    const int b1 = __builtin_ctz(later >> (b6 + 1)) + b6 + 1;
                    const uint32_t cover = ((1u << b1) - 1u) & ~((1u << b6) - 1u);
                    uint32_t d = (uint32_t)((b6 * nch + c6) * 256) | ((lfe && c6 == nch - 1) ? 1u << 14 : 0u) | (cover << 16) | ((uint32_t)(b6 * nch + c6) << 24);
                    if constexpr (CPL) d |= cplf && c6 < nfbw ? 1u << 22 : 0u;
                    L.rowdesc[__builtin_popcountll(row_set & ((1ull << lane) - 1ull))] = d;
                }
            }
            // ---- fixed side information (:880-916) ----
            {
                // what every frame of the layout sends (enc_syntax.h, with the reference's quirks); then what this frame adds
                frame_bits += syn_priced_fixed(acmod, lfe, nfbw, nch);
                // chbwcod (6 bits) and gainrng (2 bits) of every full-bandwidth channel-block that sends exponents
                uint64_t fbw_rows = 0;
                for (int b = 0; b < 6; b++) fbw_rows |= ((1ull << nfbw) - 1) << (6 * b);
                frame_bits += 8 * __builtin_popcountll(row_set & fbw_rows);
                if constexpr (DRC) if (!DW || P.drc) {
                    const uint8_t *code = P.drc + fidx * 6;
                    for (int b = 0; b < 6; b++) frame_bits += drc_sends(code, b) ? (acmod == 0 ? 16 : 8) : 0;     // (dual mono: dynrng2 too)
                }
                if constexpr (DW) {                 // each programme's own sends; compr / compr2
                    const int np = acmod == 0 ? 2 : 1;
                    if (P.dyn) {
                        const uint8_t *code = P.dyn + fidx * 12;
                        for (int b = 0; b < 6; b++)
                            for (int p = 0; p < np; p++) frame_bits += dyn_sends(code, b, p) ? 8 : 0;
                    }
                    for (int p = 0; p < np; p++) frame_bits += (compr_word(P, fidx, p) & 0x100u) ? 8 : 0;
                }
                // rematrixing: the four flags of every block 1..5 that sends them (block 0's stay uncounted)
                if (!FX && P.remat)
                    for (int b = 1; b < 6; b++) frame_bits += (P.remat[fidx * 6 + b] & 0x10) ? 4 : 0;
                if (CPL && cplf) {
                    // the coupling fields; the coupling exponents; no chbwcod for the coupled channels
                    frame_bits += syn_priced_cpl(acmod, nfbw, cpl_nb);
                    frame_bits += __builtin_amdgcn_readfirstlane(P.cpl.ebits[fidx]) - 6 * __builtin_popcountll(row_set & fbw_rows);
                    if (P.remat) {                  // a coupled frame's blocks 1..5 send liba52's cplinu-1 flag count, not 4
                        const int nrem = syn_cpl_nrem(P.cpl_begf);
                        for (int b = 1; b < 6; b++) frame_bits -= (P.remat[fidx * 6 + b] & 0x10) ? 4 - nrem : 0;
                    }
                }
            }
            if constexpr (CPL) if (cplf) {
                // the coupling rows: masks to rows 36.., run starts behind the channels' in rowdesc
                if constexpr (!WIN) {
                    const uint32_t *gm = reinterpret_cast<const uint32_t *>(P.cpl.emask + fidx * 6 * 50);
                    for (int i = lane; i < 150; i += 64) reinterpret_cast<uint32_t *>(&L.mask[36][0])[i] = gm[i];
                }
                const int st = lane < 6 ? (int)P.cpl.strat[fidx * 8 + lane] : 0;
                const uint32_t cst = (uint32_t)__ballot(lane < 6 && st != 0) | 0x40u;
                const int n0 = __builtin_popcountll(row_set);
                if (lane < 6 && st != 0) {
                    const int b1 = __builtin_ctz(cst >> (lane + 1)) + lane + 1;
                    const uint32_t cover = ((1u << b1) - 1u) & ~((1u << lane) - 1u);
                    L.rowdesc[n0 + __builtin_popcount(cst & ((1u << lane) - 1u))] = (uint32_t)(lane * 256) | (1u << 15) | (cover << 16) | ((uint32_t)(36 + lane) << 24);
                }
                ncplrows = __builtin_popcount(cst & 0x3fu);
                wave_sync();
            }
        };
        // PART 1 replays the search from tabulated verdicts and needs the frame's data only for a verdict that is missing
        // (FX has no table: its first question always costs a sweep - loaded here, no address is kept across the search loop)
        if (PART != 1 || FX || P.tap_strat) load_frame();

        // ---- SNR offset search, exactly the reference's sequence (:921-967).  PART 3: up to three candidates are
        //      evaluated per sweep over the coefficients, chosen by running the reference's loop ahead on
        //      the assumption that each one fits; the verdicts are then consumed in the reference's order
        //      and everything after the first surprise is discarded.  PART 1: a window of sixteen consecutive
        //      offsets per sweep (cost_window below), the reference's loop replayed from the verdicts it leaves. ----
        const uint32_t bandoff = *reinterpret_cast<const uint32_t *>(&L.band_of_bin[4 * lane]);    // bands of bins 4*lane..+3
        SnrSearch ss{csnr_prev, 0, 0, false};
        // Verdicts already known for this frame: bit cc of known_c / fits_c for (cc, fsnroffst 0), bit ff of
        // known_f / fits_f for (csnroffst f_cc, ff > 0).  The reference asks for some offsets twice.
        uint64_t known_c = 0, fits_c = 0;
        uint32_t known_f = 0, fits_f = 0;
        int f_cc = -1;
        if (PART == 1 && !FX && P.memo) {                                  // tabulated by PART 3
            const uint32_t *m = P.memo + fidx * 8;
            auto word = [&](int i) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)m[i]); };    // (the builtin returns int)
            known_c = (uint64_t)word(0) | ((uint64_t)word(1) << 32);
            fits_c = (uint64_t)word(2) | ((uint64_t)word(3) << 32);
            known_f = word(4);
            fits_f = word(5);
            f_cc = (int)word(6);
        }
        bool went_down = false, went_up = false;           // (the three-offset policy's: PART 3 alone reads them)
        // Verdicts that follow from a costed offset WITHOUT costing.  A frame's mantissa bits are N + E: N = the sum over the
        // coefficients of a nominal width (0, 5/3, 7/3, 3, 7/2, 4, 5 ... 16 by bap), E = what the grouped codes' ceilings add - per
        // block 10/3 or 5/3 bits for one or two 3-level mantissas left over, 14/3 or 7/3 for 5-level ones, 7/2 for an odd 11-level
        // one: 0 <= E <= 69 bits a frame.  N cannot fall when the offset rises (a coefficient's bap table address, :393-420, never
        // falls with snroffset, and the widths rise with the address).  So with the E of a COSTED offset g1 in hand (it follows from
        // the counts the sweep reduces anyway): every g > g1 spends at least N(g1) = bits(g1) - E(g1): all fail if spare(g1) <
        // -E(g1); every g < g1 spends at most N(g1) + 69: all fit if spare(g1) >= 69 - E(g1) - exactly, whatever their own ceilings
        // do.  (Rounds 2-3 used +-72 for both; the band of undecided offsets is half as wide now: profiles/search_sim.py, 3.39 ->
        // 3.22 sweeps per fresh frame, 2.57 -> 2.33 with a transcode's hint.)  Sixths of a bit; offsets as g = 16 csnroffst + fsnroffst.
        int fit_hi = -1, fail_lo = 1 << 20;
        // Every offset costed for this frame, whether the reference asks for it or not: 1024-bit maps "costed" / "fits", word w in
        // lane w of one register each; and the two costed offsets that enclose the boundary most closely, with their spare bits.
        uint32_t costed_map = 0, fits_map = 0;
        int gl = -1, spare_l = 0, gh = -1, spare_h = 0;
        int probe_sweeps = 0;                               // (PART 3 alone)
        auto lookup = [&](int cc, int ff, bool &fits) {
            const int g = 16 * cc + ff;
            if (g <= fit_hi) { fits = true; return true; }
            if (g >= fail_lo) { fits = false; return true; }
            if (((uint32_t)__builtin_amdgcn_readlane((int)costed_map, g >> 5) >> (g & 31)) & 1u) {
                fits = ((uint32_t)__builtin_amdgcn_readlane((int)fits_map, g >> 5) >> (g & 31)) & 1u;
                return true;
            }
            if (ff == 0) { fits = (fits_c >> cc) & 1; return (bool)((known_c >> cc) & 1); }
            fits = (fits_f >> ff) & 1;
            return cc == f_cc && ((known_f >> ff) & 1);
        };
        // Mantissa bits of the whole frame at up to three offsets, and the verdicts into the memo.  Bit allocation
        // is a function of the (encoded) exponents alone, so a block that reuses a channel's exponents has that
        // channel's counts of the block that sent them: every run of blocks is counted once, 64 bins per step, and
        // added to the per-lane accumulators of all blocks of the run.
        auto cost_and_record = [&](const int (&cg)[ENC_NC], int n_cand, bool probing) {
          if constexpr (!WIN) {                 // (PART 3 alone)
            if (!loaded) load_frame();
            int so[ENC_NC];                 // snroffset (:393-420) of the candidates; unused slots repeat the first
#pragma unroll
            for (int k = 0; k < ENC_NC; k++) so[k] = ((k < n_cand ? cg[k] : cg[0]) - 240) << 2;
            PK_COUNT(4);
            const int budget = 16 * fs - frame_bits;
            uint32_t acc[6][ENC_NC];
#pragma unroll
            for (int B = 0; B < 6; B++)
#pragma unroll
                for (int c = 0; c < ENC_NC; c++) acc[B][c] = 0;
            {
                // one run-start row per step: four bins per lane from one dword (HBM/L2); the exponent dwords of the next
                // three rows are in flight while one is costed
                const int nrows = __builtin_popcountll(row_set) + (CPL ? ncplrows : 0);
                auto desc_of = [&](int i) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)L.rowdesc[i < nrows ? i : nrows - 1]); };
                auto fetch = [&](uint32_t d) {
                    if constexpr (CPL) return *reinterpret_cast<const uint32_t *>(((d & (1u << 15)) ? cex : ex) + (d & 0x3fffu) + 4 * lane);
                    else return *reinterpret_cast<const uint32_t *>(ex + (d & 0x3fffu) + 4 * lane);
                };
                uint32_t d0 = desc_of(0), d1 = desc_of(1), d2 = desc_of(2);
                uint32_t ev = fetch(d0), ev1 = fetch(d1), ev2 = fetch(d2);
                static_assert(ENC_NC == 3, "two packed candidates + one");
                // a row's band terms (lane = band), a row ahead of its coefficients
                auto terms = [&](uint32_t d, int buf) {
                    const int m = L.mask[d >> 24][lane < 50 ? lane : 49];
                    int D[3];
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        int q = ((m - so[c]) >> 3) & ~3;
                        q = q < 0 ? 0 : q;
                        D[c] = 320 - q;
                    }
                    if (lane < 50) L.terms[buf][lane] = make_uint2((uint32_t)(D[0] & 0xffff) | ((uint32_t)D[1] << 16), (uint32_t)(D[2] & 0xffff));
                };
                terms(d0, 0);
                // bins the row does not code: exponent 255 - term - 16 x 255 < 0, table address 0, bap 0, no bits
                auto beyond = [&](int n) { const int k = n - 4 * lane; return k >= 4 ? 0u : k <= 0 ? 0xffffffffu : 0xffffffffu << (8 * k); };
                const uint32_t um_fbw = beyond(nbc), um_lfe = beyond(7);
                uint32_t boff[4];                                           // byte offsets of the lane's four bands in a terms buffer
#pragma unroll
                for (int j = 0; j < 4; j++) boff[j] = ((bandoff >> (8 * j)) & 0xffu) * 8u;
#pragma unroll 1
                for (int i = 0; i < nrows; i++) {
                    const uint32_t d3 = desc_of(i + 3);
                    const uint32_t ev3 = fetch(d3);
                    if (i + 1 < nrows) terms(d1, (i + 1) & 1);
                    const char *Tr = reinterpret_cast<const char *>(&L.terms[i & 1][0]);
                    uint32_t em;
                    if constexpr (CPL) {
                        const uint32_t um_cch = beyond(cpl_cs), um_cpl = ~beyond(cpl_cs) | beyond(cpl_ce);
                        em = ev | ((d0 & (1u << 14)) ? um_lfe : (d0 & (1u << 15)) ? um_cpl : (d0 & (1u << 22)) ? um_cch : um_fbw);
                    } else {
                        em = ev | ((d0 & (1u << 14)) ? um_lfe : um_fbw);
                    }
                    uint32_t sum[ENC_NC];
#pragma unroll
                    for (int c = 0; c < ENC_NC; c++) sum[c] = 0;
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const uint32_t e16 = __umul24((em >> (8 * j)) & 0xffu, 0x00100010u);           // 16 x exponent, twice
                        const uint2 t = *reinterpret_cast<const uint2 *>(Tr + boff[j]);
                        pk2 a01 = __builtin_bit_cast(pk2, t.x) - __builtin_bit_cast(pk2, e16);
                        pk2 a2 = __builtin_bit_cast(pk2, t.y) - __builtin_bit_cast(pk2, e16);
                        a01 = __builtin_elementwise_min(__builtin_elementwise_max(a01, (pk2){0, 0}), (pk2){252, 252});
                        a2 = __builtin_elementwise_min(__builtin_elementwise_max(a2, (pk2){0, 0}), (pk2){252, 252});
                        const char *lut = reinterpret_cast<const char *>(&L.bitlut[0]);
                        sum[0] += *reinterpret_cast<const uint32_t *>(lut + (uint16_t)a01.x);
                        sum[1] += *reinterpret_cast<const uint32_t *>(lut + (uint16_t)a01.y);
                        sum[2] += *reinterpret_cast<const uint32_t *>(lut + (uint16_t)a2.x);
                    }
#pragma unroll
                    for (int B = 0; B < 6; B++) {
                        const uint32_t in_run = (d0 >> (16 + B)) & 1u;               // wave-uniform
#pragma unroll
                        for (int k = 0; k < ENC_NC; k++)    // (written out: the compiler turns a multiply by 0/1 back into select + add)
                            asm("v_mad_u32_u24 %0, %1, %2, %0" : "+v"(acc[B][k]) : "v"(sum[k]), "s"(in_run));
                    }
                    d0 = d1; d1 = d2; d2 = d3;
                    ev = ev1; ev1 = ev2; ev2 = ev3;
                }
            }
            // Frame totals.  Plain bits: summed over the blocks in the lane, one reduction per candidate.  The 3/5/11-level counts
            // of a (block, candidate) pair: three 10-bit fields reduced over either half of the wavefront (32 x 24 < 1024) and
            // dropped into lane 8 c + B of two collecting registers, so that the ceilings (:1194-1238: a code per 3, 3 or 2
            // mantissas of a block) are worked out once, across lanes, instead of pair by pair on the scalar unit.
            int total[ENC_NC], extra6[ENC_NC];
            {
                uint32_t col_lo = 0, col_hi = 0, bits_l[ENC_NC];
#pragma unroll
                for (int c = 0; c < ENC_NC; c++) bits_l[c] = 0;
#pragma unroll
                for (int B = 0; B < 6; B++) {
#pragma unroll
                    for (int c = 0; c < ENC_NC; c++) {
                        const uint32_t a = acc[B][c];
                        bits_l[c] += a & 0x1ffu;
                        uint32_t v = ((a >> 9) & 31u) | (((a >> 14) & 31u) << 10) | (((a >> 19) & 31u) << 20);
                        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);
                        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);
                        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);
                        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);
                        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
                        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)v, 31), hi = (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
                        const bool mine = lane == 8 * c + B;
                        col_lo = mine ? lo : col_lo;
                        col_hi = mine ? hi : col_hi;
                    }
                }
                const uint32_t n1 = (col_lo & 1023u) + (col_hi & 1023u), n2 = ((col_lo >> 10) & 1023u) + ((col_hi >> 10) & 1023u);
                const uint32_t n4 = (col_lo >> 20) + (col_hi >> 20);
                uint32_t t = 5u * (((n1 + 2u) * 0xaaabu) >> 17) + 7u * (((n2 + 2u) * 0xaaabu) >> 17) + 7u * ((n4 + 1u) >> 1);
                // ... and the ceilings' share of them in sixths of a bit (<= 69 per block): bits << 10 | sixths ride one reduction
                t = (t << 10) | (6u * t - (10u * n1 + 14u * n2 + 21u * n4));
                t += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x111, 0xf, 0xf, true);      // lanes 8 c .. 8 c + 7 -> lane 8 c + 7
                t += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x112, 0xf, 0xf, true);
                t += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t, 0x114, 0xf, 0xf, true);
#pragma unroll
                for (int c = 0; c < ENC_NC; c++) {
                    const uint32_t tc = (uint32_t)__builtin_amdgcn_readlane((int)t, 8 * c + 7);
                    total[c] = (int)wave_sum_u32(bits_l[c]) + (int)(tc >> 10);
                    extra6[c] = (int)(tc & 1023u);
                }
            }
#pragma unroll
            for (int i = 0; i < ENC_NC; i++) {
                if (i >= n_cand) break;
                const int spare = budget - total[i];
                const bool ok = spare >= 0;
                const int g = cg[i], cand_ci = g >> 4, cand_fi = g & 15;
                if (6 * spare >= 414 - extra6[i] && g > fit_hi) fit_hi = g;
                if (6 * spare < -extra6[i] && g < fail_lo) fail_lo = g;
                {
                    const uint32_t bit = lane == (g >> 5) ? 1u << (g & 31) : 0u;
                    costed_map |= bit;
                    fits_map |= ok ? bit : 0u;
                }
                {                                   // (selects: an if / else here makes hipcc keep the four in scratch)
                    const bool up = ok && g > gl, dn = !ok && (gh < 0 || g < gh);
                    gl = up ? g : gl; spare_l = up ? spare : spare_l;
                    gh = dn ? g : gh; spare_h = dn ? spare : spare_h;
                }
                if (cand_fi == 0) { known_c |= 1ull << cand_ci; fits_c |= (uint64_t)ok << cand_ci; }
                else if (!probing || cand_ci == f_cc) {
                    if (cand_ci != f_cc) { f_cc = cand_ci; known_f = fits_f = 0; }     // costed ahead for another csnroffst
                    known_f |= 1u << cand_fi;
                    fits_f |= (uint32_t)ok << cand_fi;
                }
            }
          }
        };
        // The window sweep (snr_window.h): the frame's exact cost at the sixteen offsets lo .. lo + 15 from ONE pass over the
        // run-start rows.  Per row: the band lanes (lane = band) work out k0 and the steps t1, t2 of their band a row ahead
        // (win_steps) from the row's mask word, which they read from memory two rows ahead; every bin looks up three cost words,
        // at the addresses of k0, k0 - 1 and k0 - 2 (the same packed arithmetic as the three-offset sweep, on the terms win_term
        // + 0, 4, 8); the first goes to the blocks' accounts as before (acc: the cost at lo itself); a wave prefix sum of each word
        // over the bins - modulo 2^32, exact: packing is linear and a band's own sum fits its fields, whatever overflowed before
        // it - gives the band lanes W0, W1, W2, and these add W1 - W0 at t1 and W2 - W1 at t2 to the histogram of the run's
        // first block and take them back at the block behind the run (L.hist).  Behind the rows: lane t sums the histogram over
        // the blocks up to B and over the steps up to t, adds B's account and has the block's totals at lo + t; ceilings and
        // sixths lane-parallel (win_block_bits); the sixteen verdicts into the maps and bounds.
        // known_c / known_f are the tabulation's (PART 3 -> memo) and stay as loaded: lookup asks the maps first.
        int win_sweeps = 0, win_slope15 = 0, win_cmin = 1 << 20, win_cmax = -1;
        auto cost_window = [&](int lo) {
          if constexpr (WIN) {
            if (!loaded) load_frame();
            PK_COUNT(4);
            const int so_lo = win_snroffset(lo);
            const int budget = 16 * fs - frame_bits;
            uint32_t acc[6];
#pragma unroll
            for (int B = 0; B < 6; B++) acc[B] = 0;
            static_assert(sizeof L.hist == 180 * sizeof(uint4), "cleared as 180 uint4");
#pragma unroll
            for (int i = 0; i < 3; i++)
                if (lane + 64 * i < 180) reinterpret_cast<uint4 *>(&L.hist[0][0][0][0])[lane + 64 * i] = make_uint4(0, 0, 0, 0);
            {
                const int nrows = __builtin_popcountll(row_set) + (CPL ? ncplrows : 0);
                auto desc_of = [&](int i) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)L.rowdesc[i < nrows ? i : nrows - 1]); };
                auto fetch = [&](uint32_t d) {
                    if constexpr (CPL) return *reinterpret_cast<const uint32_t *>(((d & (1u << 15)) ? cex : ex) + (d & 0x3fffu) + 4 * lane);
                    else return *reinterpret_cast<const uint32_t *>(ex + (d & 0x3fffu) + 4 * lane);
                };
                // the row's mask word of the lane's band (rows 36 + blk: the coupling's)
                const int bl = lane < 50 ? lane : 49;
                const int16_t *gmask = P.emask + fidx * 6 * nch * 50 + bl;
                auto mask_of = [&](uint32_t d) {
                    if constexpr (CPL) if (d & (1u << 15)) return (int)P.cpl.emask[(fidx * 6 + ((d >> 24) - 36)) * 50 + bl];
                    return (int)gmask[(d >> 24) * 50u];
                };
                uint32_t d0 = desc_of(0), d1 = desc_of(1), d2 = desc_of(2);
                uint32_t ev = fetch(d0), ev1 = fetch(d1), ev2 = fetch(d2);
                int t1c = 0, t2c = 0;                   // the steps of the lane's band in the row being costed
                auto terms = [&](int m, int buf, int &t1, int &t2) {
                    int k0;
                    win_steps(m - so_lo, k0, t1, t2);
                    const int D = win_term(k0);
                    if (lane < 50) L.terms[buf][lane] = make_uint2((uint32_t)(D & 0xffff) | ((uint32_t)(D + 4) << 16), (uint32_t)((D + 8) & 0xffff));
                };
                int mv1 = mask_of(d1);
                terms(mask_of(d0), 0, t1c, t2c);
                // bins the row does not code: exponent 255 - term - 16 x 255 < 0, table address 0, bap 0, no bits
                auto beyond = [&](int n) { const int k = n - 4 * lane; return k >= 4 ? 0u : k <= 0 ? 0xffffffffu : 0xffffffffu << (8 * k); };
                const uint32_t um_fbw = beyond(nbc), um_lfe = beyond(7);
                uint32_t boff[4];                                           // byte offsets of the lane's four bands in a terms buffer
#pragma unroll
                for (int j = 0; j < 4; j++) boff[j] = ((bandoff >> (8 * j)) & 0xffu) * 8u;
#pragma unroll 1
                for (int i = 0; i < nrows; i++) {
                    const uint32_t d3 = desc_of(i + 3);
                    const uint32_t ev3 = fetch(d3);
                    const int mv2 = mask_of(d2);
                    const char *Tr = reinterpret_cast<const char *>(&L.terms[i & 1][0]);
                    uint32_t em;
                    if constexpr (CPL) {
                        const uint32_t um_cch = beyond(cpl_cs), um_cpl = ~beyond(cpl_cs) | beyond(cpl_ce);
                        em = ev | ((d0 & (1u << 14)) ? um_lfe : (d0 & (1u << 15)) ? um_cpl : (d0 & (1u << 22)) ? um_cch : um_fbw);
                    } else {
                        em = ev | ((d0 & (1u << 14)) ? um_lfe : um_fbw);
                    }
                    uint32_t p[3][4];                   // the three words, summed over the lane's bins up to j
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const uint32_t e16 = __umul24((em >> (8 * j)) & 0xffu, 0x00100010u);           // 16 x exponent, twice
                        const uint2 t = *reinterpret_cast<const uint2 *>(Tr + boff[j]);
                        pk2 a01 = __builtin_bit_cast(pk2, t.x) - __builtin_bit_cast(pk2, e16);
                        pk2 a2 = __builtin_bit_cast(pk2, t.y) - __builtin_bit_cast(pk2, e16);
                        a01 = __builtin_elementwise_min(__builtin_elementwise_max(a01, (pk2){0, 0}), (pk2){252, 252});
                        a2 = __builtin_elementwise_min(__builtin_elementwise_max(a2, (pk2){0, 0}), (pk2){252, 252});
                        const char *lut = reinterpret_cast<const char *>(&L.bitlut[0]);
                        const uint32_t v0 = *reinterpret_cast<const uint32_t *>(lut + (uint16_t)a01.x);
                        const uint32_t v1 = *reinterpret_cast<const uint32_t *>(lut + (uint16_t)a01.y);
                        const uint32_t v2 = *reinterpret_cast<const uint32_t *>(lut + (uint16_t)a2.x);
                        p[0][j] = j ? p[0][j - 1] + v0 : v0;
                        p[1][j] = j ? p[1][j - 1] + v1 : v1;
                        p[2][j] = j ? p[2][j - 1] + v2 : v2;
                    }
#pragma unroll
                    for (int B = 0; B < 6; B++) {
                        const uint32_t in_run = (d0 >> (16 + B)) & 1u;               // wave-uniform
                        asm("v_mad_u32_u24 %0, %1, %2, %0" : "+v"(acc[B]) : "v"(p[0][3]), "s"(in_run));
                    }
                    // bins -> bands: one buffer for the three words (a wavefront's LDS accesses keep their order)
                    uint32_t W[3];
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        const uint32_t incl = wave_incl_scan_u32(p[c][3]);
                        const uint32_t before = incl - p[c][3];
                        *reinterpret_cast<uint4 *>(&L.scan[4 + 4 * lane]) = make_uint4(before + p[c][0], before + p[c][1], before + p[c][2], incl);
                        W[c] = L.scan[band_hi] - L.scan[band_lo];
                    }
                    // bands -> histogram, at the run's first block and behind its last
                    {
                        const uint32_t cover = (d0 >> 16) & 0x3fu;                      // wave-uniform, a run of ones
                        const int b_in = __builtin_ctz(cover), b_out = b_in + __builtin_popcount(cover);
                        const uint32_t a0 = win_wide_a(W[0]), a1 = win_wide_a(W[1]), a2 = win_wide_a(W[2]);
                        const uint32_t b0 = win_wide_b(W[0]), b1 = win_wide_b(W[1]), b2 = win_wide_b(W[2]);
                        // (no lane adds where nothing steps inside the window: the many lanes of a quiet row would meet on one address)
                        // ... nor where the step changes nothing: neighbouring table addresses mostly hold the same bap)
                        const bool s1 = lane < 50 && t1c < WIN_N && ((a1 ^ a0) | (b1 ^ b0)) != 0, s2 = lane < 50 && t2c < WIN_N && ((a2 ^ a1) | (b2 ^ b1)) != 0;
                        uint32_t *h1 = &L.hist[lane & 3][b_in][s1 ? t1c - 1 : 0][0], *h2 = &L.hist[lane & 3][b_in][s2 ? t2c - 1 : 0][0];
                        if (s1) { atomicAdd(h1, a1 - a0); atomicAdd(h1 + 1, b1 - b0); }
                        if (s2) { atomicAdd(h2, a2 - a1); atomicAdd(h2 + 1, b2 - b1); }
                        if (b_out < 6) {                                                // wave-uniform
                            const int behind = (b_out - b_in) * 30;
                            if (s1) { atomicAdd(h1 + behind, a0 - a1); atomicAdd(h1 + behind + 1, b0 - b1); }
                            if (s2) { atomicAdd(h2 + behind, a1 - a2); atomicAdd(h2 + behind + 1, b1 - b2); }
                        }
                    }
                    // the next row's terms and steps, behind this row's last use of its own (two registers fewer than a row ahead)
                    if (i + 1 < nrows) terms(mv1, (i + 1) & 1, t1c, t2c);
                    d0 = d1; d1 = d2; d2 = d3;
                    ev = ev1; ev1 = ev2; ev2 = ev3;
                    mv1 = mv2;
                }
            }
            // Frame totals at lo + t in lane t (every row of sixteen lanes the same)
            int spare, extra6;
            {
                const int t = lane & 15;
                uint32_t run_a = 0, run_b = 0, total = 0, x6 = 0;
#pragma unroll
                for (int B = 0; B < 6; B++) {
                    const uint32_t base_a = wave_sum_u32(win_wide_a(acc[B])), base_b = wave_sum_u32(win_wide_b(acc[B]));
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        const uint2 h = *reinterpret_cast<const uint2 *>(&L.hist[c][B][t ? t - 1 : 0][0]);
                        run_a += t ? h.x : 0u;
                        run_b += t ? h.y : 0u;
                    }
                    uint32_t e6;
                    total += win_block_bits(base_a + row_incl_scan_u32(run_a), base_b + row_incl_scan_u32(run_b), e6);
                    x6 += e6;
                }
                spare = budget - (int)total;
                extra6 = (int)x6;
            }
            {
                const uint32_t fits16 = (uint32_t)__ballot(spare >= 0) & 0xffffu, fails16 = fits16 ^ 0xffffu;
                const uint32_t sure_fit = (uint32_t)__ballot(6 * spare >= 414 - extra6) & 0xffffu;
                const uint32_t sure_fail = (uint32_t)__ballot(6 * spare < -extra6) & 0xffffu;
                const int g_fit = sure_fit ? lo + 31 - __builtin_clz(sure_fit) : -1, g_fail = sure_fail ? lo + __builtin_ctz(sure_fail) : 1 << 20;
                fit_hi = g_fit > fit_hi ? g_fit : fit_hi;
                fail_lo = g_fail < fail_lo ? g_fail : fail_lo;
                {                                   // sixteen bits from bit lo of the 1024-bit maps: word lo >> 5 and, past bit 16 of it, the next
                    const uint64_t c16 = (uint64_t)0xffffu << (lo & 31), f16 = (uint64_t)fits16 << (lo & 31);
                    const int w = lo >> 5;
                    costed_map |= lane == w ? (uint32_t)c16 : lane == w + 1 ? (uint32_t)(c16 >> 32) : 0u;
                    fits_map |= lane == w ? (uint32_t)f16 : lane == w + 1 ? (uint32_t)(f16 >> 32) : 0u;
                }
                {                                   // the costed offsets that enclose the boundary most closely (selects, as above)
                    const int il = fits16 ? 31 - __builtin_clz(fits16) : 0, ih = fails16 ? __builtin_ctz(fails16) : 0;
                    const int sp_l = __builtin_amdgcn_readlane(spare, il), sp_h = __builtin_amdgcn_readlane(spare, ih);
                    const bool up = fits16 && lo + il > gl, dn = fails16 && (gh < 0 || lo + ih < gh);
                    gl = up ? lo + il : gl; spare_l = up ? sp_l : spare_l;
                    gh = dn ? lo + ih : gh; spare_h = dn ? sp_h : spare_h;
                }
                win_slope15 = __builtin_amdgcn_readlane(spare, 0) - __builtin_amdgcn_readlane(spare, 15);
                win_cmin = lo < win_cmin ? lo : win_cmin;
                win_cmax = lo + 15 > win_cmax ? lo + 15 : win_cmax;
                if constexpr (!FX) if (P.tap_curve && lane < WIN_N) {
                    P.tap_curve[(fidx * 1024 + lo + lane) * 2] = spare;
                    P.tap_curve[(fidx * 1024 + lo + lane) * 2 + 1] = extra6;
                }
            }
          }
        };
        bool first_sweep = true;                            // (PART 3 alone; the window loop counts win_sweeps)
        const bool cold_hint = csnr_prev == 40 && fsnr_prev == 0;          // the state AC3_encode_init leaves (a guess that only steers which offsets are costed first)
        if constexpr (WIN) {
            // Windows until the verdicts answer every question of the reference's loop: the first around the source frame's
            // offsets (a transcode), where fresh material lands (a cold stream) or around the stream's last offsets; the next where
            // the line through the enclosing costed offsets crosses zero, along the last window's slope while only one side is
            // known, then by halving, at last around the open question itself (win_first_lo / win_next_lo; sweeps per frame:
            // profiles/search_window_sim.py)
            for (;;) {
                int cc, ff;
                bool more;
                while ((more = ss.next(cc, ff))) {
                    bool fits;
                    if (!lookup(cc, ff, fits)) break;
                    ss.consume(fits);
                }
                if (!more) break;
                int lo;
                if (win_sweeps == 0) {
                    const int hint0 = (cold_hint && P.hint) ? (int)__builtin_amdgcn_readfirstlane((int)P.hint[fidx * (size_t)P.hint_stride]) : 0;    // (0: no hint)
                    lo = win_first_lo(hint0, cold_hint, 16 * csnr_prev + fsnr_prev);
                } else {
                    lo = win_next_lo(win_sweeps, gl, spare_l, gh, spare_h, win_slope15, win_cmin, win_cmax, 16 * cc + ff);
                }
                win_sweeps++;
                cost_window(lo);
            }
        } else
        for (;;) {
            // advance the reference's loop as far as the known verdicts reach
            int cc, ff;
            bool more;
            while ((more = ss.next(cc, ff))) {
                bool fits;
                if (!lookup(cc, ff, fits)) break;
                if (ss.phase == 0 && !fits) went_down = true;
                if (ss.phase == 1 && fits) went_up = true;
                ss.consume(fits);
            }
            if (!more) break;
            // up to three offsets not costed yet, along the likeliest continuation: the start value fits unless
            // an earlier one did not, +4 steps fail unless one has fitted, the finer steps fit
            // (candidates as g = 16 csnroffst + fsnroffst in a list written through static indices only: a dynamic index sends
            // such arrays to scratch)
            int cg[ENC_NC], n_cand = 0;
#pragma unroll
            for (int k = 0; k < ENC_NC; k++) cg[k] = -1;
            auto add = [&](int g) {                 // false: already in the list
                bool dup = false;
#pragma unroll
                for (int k = 0; k < ENC_NC; k++) dup = dup || cg[k] == g;
                if (dup) return false;
#pragma unroll
                for (int k = 0; k < ENC_NC; k++) cg[k] = k == n_cand ? g : cg[k];
                n_cand++;
                return true;
            };
            // While the boundary is only known to lie between two costed offsets more than three steps apart, the next offsets
            // to cost are chosen where the line through their spare bits crosses zero (and one step - a twelfth of a wide
            // bracket - either side): the monotone bounds then answer every rung the reference asks about outside the new
            // bracket.  profiles/search_sim.py replays the policies on the oracle's spare-bit curves: 5.0 -> 3.7 sweeps per cold
            // frame, 3.0 -> 2.4 per warm one.
            bool probing = false;
            if (probe_sweeps < 3 && gl >= 0 && gh > gl + 3) {
                const int w = gh - gl;
                const float est = (float)w * ((float)spare_l / (float)(spare_l - spare_h));       // relative to gl
                int d = w > 48 ? (w * 85) >> 10 : 1;
                d = d < 2 && w > 48 ? 2 : d;
                const int ge = gl + (int)(est + 0.5f);
                auto clampg = [&](int g) { return g < gl + 1 ? gl + 1 : g > gh - 1 ? gh - 1 : g; };
                add(clampg(ge));
                add(clampg(ge + d));
                add(clampg(ge - d));
                // candidates that clamped onto each other (an estimate at the bracket's edge): the nearest uncosted neighbours
                // take their places - a sweep costs the same with one offset or three (2.35 -> 2.29 sweeps per transcoded frame,
                // 3.23 -> 3.16 per fresh one, and the tails shorter: profiles/search_sim.py)
                for (int k = 1; n_cand < ENC_NC && k < w; k++) {
                    if (ge - k > gl && ge - k < gh) add(ge - k);
                    if (n_cand < ENC_NC && ge + k > gl && ge + k < gh) add(ge + k);
                }
                probe_sweeps++;
                probing = true;
            }
            // Phase 0 of a search that has to come down a long way (a fresh stream starts at 40): the ladder csnroffst,
            // csnroffst - 4, ... is probed at three points that cut its unknown stretch into quarters instead of walked three
            // rungs per sweep - the bounds above turn a rung that fails or fits by a margin into the verdict of every rung
            // beyond it.  (Which offsets are COSTED never changes a result: the reference's sequence is replayed from exact
            // verdicts only.)
            const int hint0 = (first_sweep && cold_hint && P.hint) ? (int)__builtin_amdgcn_readfirstlane((int)P.hint[fidx * (size_t)P.hint_stride]) : 0;
            if (n_cand == 0 && hint0 > 0) {                      // (0: the source frame's first block failed to parse - no hint)
                // a transcode: decoded audio re-encoded at its source's rate lands within -5 .. +11 steps of the offsets the source
                // frame carried: the first sweep costs around them - 3.4 -> 2.45 sweeps per frame (profiles/search_sim.py on
                // second-generation content).  A hint far off (another target rate) costs a sweep; results never depend on it.
                const int g0 = hint0 < 8 ? 8 : hint0 > 1000 ? 1000 : hint0;
                add(g0 - 8); add(g0 + 2); add(g0 + 12);
            }
            if (n_cand == 0 && first_sweep && cold_hint) {
                // a fresh stream's first sweep: csnroffst 8, 13 and 20, around where material lands at the usual rates (64 kbps
                // mono to 640 kbps 5.1: boundary at 8 .. 16 1/2 in profiles/search_sim.py) - 3.8 -> 3.5 sweeps per cold frame
                // against quartering 0 .. 40, no worse at the extremes
                add(16 * 8); add(16 * 13); add(16 * 20);
            }
            if (n_cand == 0 && ss.phase == 0 && (went_down || (first_sweep && cold_hint))) {
                int n = 0;
                for (int c = ss.csnr; c >= 0 && n < 16; c -= 4, n++) { bool f; if (lookup(c, 0, f)) break; }
                if (n > 3) {
                    add(16 * (ss.csnr - 4 * ((n - 1) / 4)));
                    add(16 * (ss.csnr - 4 * ((n - 1) / 2)));
                    add(16 * (ss.csnr - 4 * ((3 * (n - 1) + 2) / 4)));
                }
            }
            first_sweep = false;
            if (n_cand == 0) {
                SnrSearch ahead = ss;
                while (n_cand < ENC_NC && ahead.next(cc, ff)) {
                    bool fits;
                    if (!lookup(cc, ff, fits)) {
                        if (!add(16 * cc + ff)) break;
                        fits = ahead.phase == 0 ? !went_down : ahead.phase == 1 ? went_up : true;
                    }
                    ahead.consume(fits);
                }
            }
            cost_and_record(cg, n_cand, probing);
        }
        if (PART == 3) {
            // Tabulation for the replay (PART 1), whose start value is the previous frame's result, not this pass's:
            // every csnroffst within reach of this frame's own optimum, so that the replay finds its questions
            // answered unless the fit is not monotone around here or the level jumps between frames.
            const int C = ss.failed ? 0 : ss.csnr;
            for (;;) {
                int cg[ENC_NC], n_cand = 0;
#pragma unroll
                for (int k = 0; k < ENC_NC; k++) cg[k] = -1;
                for (int c = C - 7 < 0 ? 0 : C - 7; c <= (C + 8 > 63 ? 63 : C + 8) && n_cand < ENC_NC; c++) {
                    if ((known_c >> c) & 1) continue;
#pragma unroll
                    for (int k = 0; k < ENC_NC; k++) cg[k] = k == n_cand ? 16 * c : cg[k];
                    n_cand++;
                }
                if (n_cand == 0) break;
                cost_and_record(cg, n_cand, false);
            }
            if (lane == 0) {
                uint32_t *m = P.memo + fidx * 8;
                m[0] = (uint32_t)known_c; m[1] = (uint32_t)(known_c >> 32);
                m[2] = (uint32_t)fits_c; m[3] = (uint32_t)(fits_c >> 32);
                m[4] = known_f; m[5] = fits_f; m[6] = (uint32_t)f_cc; m[7] = 0;
            }
            continue;
        }
        int csnr = ss.csnr, fsnr = ss.fsnr;
        int failed_alloc = -1;
        {
            if (!ss.failed) { csnr_prev = csnr; fsnr_prev = fsnr; }
            else {
                // The reference's error path ("Yack, Error !!!", :930-933), reached when the start value and every start value
                // minus a multiple of 4 down to 0..3 fail - even if an offset in between would fit: compute_bit_allocation
                // returns without touching s->csnroffst / s->fsnroffst, its caller ignores the result (:1752), the header
                // carries the previous frame's offsets and the mantissas follow the allocation of the LAST attempt,
                // (start & 3, 0).  Such a frame overflows; the reference writes on, the engine drops what is beyond its buffer.
                failed_alloc = csnr_prev & 3;
                csnr = csnr_prev;
                fsnr = fsnr_prev;
            }
        }
        if (!FX && P.tap_snr && lane == 0) { P.tap_snr[fidx * 2] = csnr; P.tap_snr[fidx * 2 + 1] = fsnr; }
        if (!FX && P.tap_strat && lane < 36) {
            const int b = lane / 6, ch = lane - 6 * b;
            if (ch < nch) P.tap_strat[(fidx * 6 + b) * nch + ch] = L.strat[b][ch];
        }
        // the packer of this frame is another wavefront (enc_packf_kernel) or workgroup (enc_packb_kernel)
        if (lane == 0) { P.snr[fidx * 2] = csnr; P.snr[fidx * 2 + 1] = fsnr | (failed_alloc >= 0 ? 0x100 | (failed_alloc << 9) : 0); }
        PK_LAP(0);
    }
    if (PART == 1 && lane == 0) P.csnr_state[sslot] = csnr_prev | (fsnr_prev << 8);
    PK_END();
}



// ---------------------------------------------------------------------------------------------
// enc_packf_kernel: a frame whose SNR offsets are known (P.snr, from enc_search_kernel<1>) is packed by ONE wavefront -
// the packer of large batches.  Header, side information and exponent groups as wave-uniform fields through a 64-bit
// scalar accumulator - or, for the 5.1 frame without tools, from images by lanes (IMG below) - the mantissas block by block
// on enc_mant.h, both CRCs, the frame out.
// The six blocks' side information as images (enc_syntax.h: SynImages51), left here once per frame by lanes 0..5 (lane = block):
// 152 bytes (160 with the alignment), with which a 384 kbps frame's workgroup takes 9 744 bytes of LDS - still 16 per CU.
struct PackfImages {
    alignas(16) uint16_t at[6][8];      // per block: absexp_at of rows 0..5, suf_at, bits
    uint32_t pre[6][2];
    uint32_t suf0[2];                   // block 0's suffix (the other blocks': four zero bits, nothing to write)
};
struct PackfNoImages {};
template <bool CPL, bool IMG = false>
struct alignas(16) PackfLDS : std::conditional_t<IMG, PackfImages, PackfNoImages> {
    int16_t mask[CPL ? 7 : 6][50];  // this block's masking curves as band terms (mant_band_terms), one row per channel (+ coupling)
    uint4 packlut[64];                  // mant_pack_entry per bap table address
    alignas(16) uint16_t glist[GL_ENTRIES];
    alignas(4) uint8_t erow[256];       // encoded exponents of the channel whose exponent groups are being packed
    alignas(4) uint16_t crc_tab[256];
    // (the frame itself, MSB-first dwords + 256 bytes of headroom for the overshoot quirk, is dynamic LDS: PackParams::frw)
};

#ifndef ENC_PACK2_LB
#define ENC_PACK2_LB 4           // <true>: 124 VGPRs, no scratch (<true, false, true>: 10 VGPRs spilled, the coupled ones none).  5 per SIMD cannot
                                 // be reached any more: with the 1-KiB quantiser table a 384 kbps frame's workgroup takes ~9.7 KB of LDS, 16 per CU
                                 // (round 4, before the table: 1.78 ms per 65 536 frames at 4 against 1.84 at 5)
#endif
// FIXED51: the 5.1 configuration (five full-bandwidth channels + LFE, acmod 7) as compile-time constants - the shape large batches
// have; its five mantissa passes, the merged LFE lanes and the side information's field list then need no tests
// CPL: coupled frames (channel coupling on, never with FIXED51): the coupling fields, exponents and mantissa pass
// BW (ac3mi_set_encode_bandwidth 1 or 2): FIXED51 with the run-time nbc; CPL with the coupling range ending at cplendmant =
// 73 + 12 P.cpl_endf (3 + cpl_endf - cpl_begf bands, cplendf = P.cpl_endf)
// MD (ac3mi_set_encode_metadata / _frames / _source, ac3mi_set_encode_drc): the BSI fields of P.bsi or of the frame's own word
// (pack_bsi), and the dynrng words of P.drc if it is set
// DUAL (dual mono, acmod 0; generic and uncoupled only): the second programme's BSI fields and dynrng2e / dynrng2
// DW (with MD; ac3mi_set_encode_dynrng_frames / ac3mi_set_encode_drc_source): compre / compr (compr2e / compr2) of P.compr, and
// the dynrng words of P.dyn - each programme's own, sent by dyn_sends - when it is set, else P.drc's as above
template <bool FIXED51, bool CPL = false, bool BW = false, bool MD = false, bool DUAL = false, bool DW = false>
__global__ __launch_bounds__(64, ENC_PACK2_LB) void enc_packf_kernel(const PackParams P)
{
    static_assert(!DW || MD, "the array words are written where the profiles' are");
    static_assert(!(FIXED51 && CPL), "coupled frames take the generic packer");
    static_assert(!(DUAL && (FIXED51 || CPL)), "dual mono is neither 5.1 nor coupled");
    // IMG: the 5.1 frame without tools - its side information from images (syn_block_images_51), placed by lanes
    constexpr bool IMG = FIXED51 && !CPL && !MD && !DUAL && !DW;
    __shared__ PackfLDS<CPL, IMG> L;
    extern __shared__ uint4 pk_dyn[];
    uint32_t *fr = reinterpret_cast<uint32_t *>(pk_dyn);
    const int lane = threadIdx.x;
    PK_DECL();

    // (loop kept.  Copying the table as dwords measured 4 % SLOWER in round 3 - code placement, not work.  Measured again as four
    // 16-bit loads a lane issued with every other set-up load ahead of ONE wait instead of a wait per turn: 1.584 -> 1.574 ms per
    // 65 536 frames, inside the traces' standard deviation of 0.03 - no gain to keep: profiles/EXPERIMENTS.md, set-up loads)
    for (int i = lane; i < 256; i += 64) L.crc_tab[i] = P.tab->crc_tab[i];
    {
        const int bp = P.tab->baptab[lane];
        L.packlut[lane] = mant_pack_entry(bp, plain_bits(bp));
    }
    mant_lists_init(L.glist, lane);
    const uint32_t bandoff = *reinterpret_cast<const uint32_t *>(&P.tab->band_of_bin[4 * lane]);     // bands of bins 4*lane..+3
    const int nch = FIXED51 ? 6 : P.nch, nfbw = FIXED51 ? 5 : P.nfbw, nbc = FIXED51 && !BW ? 223 : P.nbc;
    const int acmod = FIXED51 ? 7 : P.acmod;
    const bool lfe = FIXED51 ? true : P.lfe != 0;
    const int fs = P.frame_words;
    // (One wavefront per frame, on purpose.  A persistent grid - 16 wavefronts per CU walking the frames, tables set up once per
    // wavefront - was measured in round 4: 2.06 ms per 65 536 frames against 1.76; with the loop but one frame per wavefront
    // 1.84.  Wavefronts that start together stay in step - all in their scalar side information, then all in their mantissa
    // passes - and the units they share are used in turns instead of side by side; the dispatcher's staggered starts mix the phases.)
    const size_t fidx = blockIdx.x;
    // channel coupling (enc_cpl_kernel): every full-bandwidth channel in coupling, one set of coordinates in block 0
    const uint32_t cplw = CPL ? (uint32_t)__builtin_amdgcn_readfirstlane((int)P.cpl.word[fidx]) : 0u;
    const bool cplf = (cplw & 1u) != 0;
    const int cs = 37 + 12 * P.cpl_begf;
    const int cendf = BW ? P.cpl_endf : 12, ce = 73 + 12 * cendf;
    PK_T0();
    PK_COUNT(7);
    for (int i = lane; i < P.frw / 4; i += 64) reinterpret_cast<uint4 *>(fr)[i] = make_uint4(0, 0, 0, 0);
    const int32_t *md = P.mdct + fidx * 6 * nch * 256;
    const uint8_t *ex = P.eexp + fidx * 6 * nch * 256;
    // lane 6 b + ch: exponent strategy and exp_samples of channel ch in block b
    int strat_l = 0, shift_l = 0;
    if (lane < 36) {
        const int b = lane / 6, ch = lane - 6 * b;
        if (ch < nch) { strat_l = (int)P.strat[(fidx * 6 + b) * nch + ch]; shift_l = (int)P.shift[(fidx * 6 + b) * nch + ch]; }
    }
    int csnr, fsnr, snroffset;
    {
        const int w1 = __builtin_amdgcn_readfirstlane(P.snr[fidx * 2 + 1]);
        csnr = __builtin_amdgcn_readfirstlane(P.snr[fidx * 2]);
        fsnr = w1 & 15;
        snroffset = (((csnr - 15) << 4) + fsnr) << 2;
        if (w1 & 0x100) snroffset = (((w1 >> 9) - 15) << 4) << 2;       // a frame whose search failed: the last attempt's allocation under the stale header offsets
    }
    if constexpr (IMG) {
        // lane b: block b's images and row offsets, from the strategies' two bit planes (lane 6 b + ch: bit 6 b + ch)
        const uint64_t s_lo = __ballot(strat_l & 1), s_hi = __ballot(strat_l & 2);
        if (lane < 6) {
            const uint32_t lo = (uint32_t)(s_lo >> (6 * lane)) & 63u, hi = (uint32_t)(s_hi >> (6 * lane)) & 63u;
            uint32_t bswm = 0;
            if (P.bsw) {
#pragma unroll
                for (int ch = 0; ch < 5; ch++) bswm = (bswm << 1) | P.bsw[(fidx * 6 + lane) * 6 + ch];
            }
            SynImages51 im;
            syn_block_images_51(im, lane, bswm, [&](int ch) { return ((lo >> ch) & 1u) | (((hi >> ch) & 1u) << 1); }, nbc, (uint32_t)P.chbwcod,
                                (uint32_t)csnr, (uint32_t)fsnr);
            *reinterpret_cast<uint4 *>(L.at[lane]) = make_uint4((uint32_t)(im.absexp_at[0] | im.absexp_at[1] << 16), (uint32_t)(im.absexp_at[2] | im.absexp_at[3] << 16),
                                                                (uint32_t)(im.absexp_at[4] | im.absexp_at[5] << 16), (uint32_t)(im.suf_at | im.bits << 16));
            *reinterpret_cast<uint2 *>(L.pre[lane]) = make_uint2(im.pre[0], im.pre[1]);
            if (lane == 0) *reinterpret_cast<uint2 *>(L.suf0) = make_uint2(im.suf[0], im.suf[1]);
        }
    }
    wave_sync();
    PK_LAP(6);

    // ---- header (:1113-1147) ----
    // Side information is wave-uniform: the field lists of enc_syntax.h through its 64-bit accumulator (PackSink), which stays
    // in scalar registers - but for the 5.1 frame without tools (IMG), whose header is one image stored by three lanes.
    uint32_t pos;                       // first bit not yet in the frame
    if constexpr (IMG) {
        uint32_t hw[3];
        syn_header_image_51(hw, (uint32_t)P.fscod, (uint32_t)P.frmsizecod, (uint32_t)P.bsid, BSI_DEFAULT);
        if (lane < 3) fr[lane] = lane == 0 ? hw[0] : lane == 1 ? hw[1] : hw[2];
        pos = SYN_HEADER_BITS_51;
    } else {
        PackSink k(fr, P.frw, lane, L.erow, [](int) { return 0u; }, cs, 0u);
        syn_header(k, P.fscod, P.frmsizecod, P.bsid, acmod, lfe, DUAL, MD ? pack_bsi(P, fidx) : BSI_DEFAULT,
                   DW ? compr_word(P, fidx, 0) : 0u, DW && DUAL ? compr_word(P, fidx, 1) : 0u);
        pos = k.pos;
    }
    const SynShape shape{acmod, nfbw, nch, lfe, DUAL, nbc, (uint32_t)P.chbwcod};

    // ---- audio blocks (:1194-1502) ----
#pragma unroll 1
    for (int b = 0; b < 6; b++) {
        // this block's encoded exponents, one dword (four bins) per lane and channel, all rows in flight together: the
        // mantissa passes use them from registers, the exponent groups of a channel through L.erow
        uint32_t ew[6];
#pragma unroll
        for (int ch = 0; ch < 6; ch++) ew[ch] = ch < nch ? *reinterpret_cast<const uint32_t *>(ex + ((size_t)b * nch + ch) * 256 + 4 * lane) : 0u;
        uint32_t cew = 0;
        int cstg = 0;
        if (cplf) {
            cew = *reinterpret_cast<const uint32_t *>(P.cpl.eexp + (fidx * 6 + b) * 256 + 4 * lane);
            cstg = __builtin_amdgcn_readfirstlane((int)P.cpl.strat[fidx * 8 + b]);
            if (lane < 25)
                reinterpret_cast<uint32_t *>(&L.mask[CPL ? 6 : 0][0])[lane] =
                    mant_band_terms(reinterpret_cast<const uint32_t *>(P.cpl.emask + (fidx * 6 + b) * 50)[lane], snroffset);
        }
        {                                           // this block's mask rows (25 dwords per channel), in flight during the side information
            const uint32_t *gm = reinterpret_cast<const uint32_t *>(P.emask + (fidx * 6 + b) * nch * 50);
            uint32_t mv[3];
#pragma unroll
            for (int j = 0; j < 3; j++) mv[j] = lane + 64 * j < nch * 25 ? gm[lane + 64 * j] : 0u;
#pragma unroll
            for (int j = 0; j < 3; j++)
                if (lane + 64 * j < nch * 25) reinterpret_cast<uint32_t *>(&L.mask[0][0])[lane + 64 * j] = mant_band_terms(mv[j], snroffset);
        }
        auto strat_of = [&](int ch) { return (uint32_t)__builtin_amdgcn_readlane(strat_l, 6 * b + ch); };
        if constexpr (IMG) {
            // the block's fields from its images: three lanes OR the prefix in at `pos` (block 0: three more the suffix at
            // suf_at), and every row's group lanes write at the row's offset - no field goes through an accumulator, and
            // nothing between two rows waits for lane 0.  (gainrng is 0: its two bits are the frame's zeros.)
            const uint4 atw = *reinterpret_cast<const uint4 *>(L.at[b]);
            or_image(fr, P.frw, L.pre[b], pos, lane);
#pragma unroll
            for (int ch = 0; ch < 6; ch++) {
                const int stg = (int)strat_of(ch);
                if (stg == 0) continue;
                const uint32_t pair = ch < 2 ? atw.x : ch < 4 ? atw.y : atw.z;
                exp_row_at(fr, P.frw, L.erow, ew[ch], pos + ((ch & 1) ? pair >> 16 : pair & 0xffffu), stg, syn_exp_groups(ch == 5 ? 7 : nbc, stg), lane);
            }
            if (b == 0) or_image(fr, P.frw, L.suf0, pos + (atw.w & 0xffffu), lane);
            pos += (uint32_t)__builtin_amdgcn_readfirstlane((int)(atw.w >> 16));
        } else {
            const uint8_t *bs = P.bsw ? P.bsw + (fidx * 6 + b) * nch : nullptr;
            PackSink k(fr, P.frw, lane, L.erow, [&](int row) { return pick_row(ew, row, cew); }, cs, pos);
            syn_block(k, shape, SynCpl{cplw, P.cpl_begf, cendf, (uint32_t)cstg}, b,
                      [&](int ch) -> uint32_t { return bs ? bs[ch] : 0u; },
                      [&](int p) { return pack_dynrng<MD, DW>(P, fidx, b, p); },
                      acmod == 2 && P.remat ? (uint32_t)P.remat[fidx * 6 + b] : b == 0 ? 0x10u : 0u, strat_of,
                      [&](int ch, int bd) -> uint32_t { return P.cpl.co[fidx * 80 + ch * 16 + bd]; }, (uint32_t)csnr, (uint32_t)fsnr);
            pos = k.pos;
        }
        PK_LAP(1);

        // ---- mantissas (:1341-1501): enc_mant.h ----
        {
            int shv[6];
#pragma unroll
            for (int ch = 0; ch < 6; ch++) shv[ch] = __builtin_amdgcn_readlane(shift_l, 6 * b + ch);
            if (CPL && cplf) {
                MantBlock B;
                B.fr = fr; B.frw = P.frw; B.glist = L.glist; B.packlut = L.packlut;
                B.mdb = md + (size_t)b * nch * 256;
                B.tap_bap = P.tap_bap ? P.tap_bap + (fidx * 6 + b) * nch * 256 : nullptr;
                B.nch = nch; B.nbc = nbc; B.lfe = lfe; B.marker = (uint32_t)P.marker;
                // per pass: channel 0, the coupling row, channels 1.. (bins below cplstrtmant / in [cplstrtmant, cplendmant)), LFE at 6
                const int csh = __builtin_amdgcn_readfirstlane((int)P.cpl.shift[fidx * 8 + b]);
                auto beyond = [&](int n) { const int k = n - 4 * lane; return k >= 4 ? 0u : k <= 0 ? 0xffffffffu : 0xffffffffu << (8 * k); };
                const uint32_t um_cch = beyond(cs), um_cpl = ~beyond(cs) | beyond(ce), um_lfe = beyond(7);
                uint32_t ad7[7], em7[7];
                int sh7[7], neg = 0;
#pragma unroll
                for (int p = 0; p < 7; p++) {
                    const int c = p == 0 ? 0 : p == 6 ? nch - 1 : p - 1;
                    const bool on = p == 1 || (p == 6 ? lfe : p == 0 || p - 1 < nfbw);
                    uint32_t e = 0;
                    int sv = 0, trow = 0;
#pragma unroll
                    for (int c2 = 0; c2 < 6; c2++) { e = c2 == c ? ew[c2] : e; sv = c2 == c ? shv[c2] : sv; }
                    trow = c;
                    if (p == 1) { e = cew; sv = csh; trow = 6; }
                    ad7[p] = 0; em7[p] = 0; sh7[p] = sv;
                    if (on) {
                        em7[p] = e | (p == 1 ? um_cpl : p == 6 ? um_lfe : um_cch);
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            const int xe = (int)((em7[p] >> (8 * j)) & 0xff);
                            int a = (int)L.mask[trow][(bandoff >> (8 * j)) & 0xff] - 4 * xe;
                            a = a < 0 ? 0 : a > 63 ? 63 : a;
                            ad7[p] |= (uint32_t)a << (8 * j);
                            neg |= xe - sv;
                        }
                    }
                }
                PK_LAP(8);
                B.cplrow = P.cpl.mdct + (fidx * 6 + b) * 256;
                pos = mant_pack_block<true>(B, em7, ad7, sh7, __ballot(neg < 0) != 0, pos, lane);
            } else {
                uint32_t ad[6];
                int neg;
                uint32_t em[6];
                mant_block_addresses(ad, em, neg, ew, shv, L.mask, bandoff, nch, nbc, lfe, lane);
                PK_LAP(8);
                MantBlock B;
                B.fr = fr; B.frw = P.frw; B.glist = L.glist; B.packlut = L.packlut;
                B.mdb = md + (size_t)b * nch * 256;
                B.tap_bap = P.tap_bap ? P.tap_bap + (fidx * 6 + b) * nch * 256 : nullptr;
                B.nch = nch; B.nbc = nbc; B.lfe = lfe; B.marker = (uint32_t)P.marker;
                pos = mant_pack_block(B, em, ad, shv, __ballot(neg < 0) != 0, pos, lane);
            }
        }
        PK_LAP(2);
    }

    // ---- frame end (:1599-1638): bytes past 2*fs are dropped, CRCs stored over whatever is there ----
    // (the reference only zero-pads when the data is short; data bits beyond byte 2*fs-2 stay and are then overwritten by
    // crc2 - its own overshoot quirk)
    const uint32_t crcs = frame_crcs(L, fr, P, fs, lane);
    wave_sync();
    if (lane == 0) {
        fr[0] = (fr[0] & 0xffff0000u) | (crcs & 0xffff);                      // bytes 2,3
        const int p = 2 * fs - 2;                                                 // even -> inside one dword
        const int shft = 16 - 8 * (p & 3);
        fr[p >> 2] = (fr[p >> 2] & ~(0xffffu << shft)) | ((crcs >> 16) << shft);
    }
    wave_sync();
    uint8_t *dst = P.frames + fidx * P.frame_stride;
    for (int i = lane; i < (2 * fs + 3) / 4; i += 64) {
        uint32_t v = __builtin_bswap32(fr[i]);
        const int rem = 2 * fs - 4 * i;
        if (rem >= 4) *reinterpret_cast<uint32_t *>(dst + 4 * i) = v;
        else for (int k = 0; k < rem; k++) dst[4 * i + k] = (uint8_t)(v >> (8 * k));
    }
    PK_LAP(3);
    PK_END();
}

// ---------------------------------------------------------------------------------------------
// enc_packb_kernel: a frame whose SNR offsets are known (P.snr, from enc_search_kernel<1>) is packed by a workgroup of six
// wavefronts, one per AUDIO BLOCK.  Nothing but its first bit ties a block to the blocks before it, and that follows from
// bit COUNTS: every wavefront first counts its block (side information from the strategies, mantissas from one table look-up
// per coefficient), the counts meet in LDS, then all six pack at once into the frame they share (fields reach it by LDS
// atomics, so neighbours may write into one dword); both CRCs on one wavefront (crc_lanes.h); 384 lanes store the frame.
// The reference's merged-code marker quirk (a grouped code whose value equals 128 is not written, :1466-1480) shortens a
// block, i.e. moves every later block: any wavefront that meets one reports it, and the workgroup packs the frame once more
// with those fields at width 0 - as enc_pack_kernel does per block.

struct PackbWave {                  // per wavefront = audio block
    int16_t mask[6][50];            // masking curves of the block's channels as band terms (mant_band_terms)
    alignas(16) uint16_t glist[GL_ENTRIES];     // members of the block's grouped codes (enc_mant.h)
    alignas(4) uint8_t erow[256];
};
struct alignas(16) PackbLDS {
    PackbWave w[6];
    uint4 packlut[64];
    uint16_t crc_tab[256];
    uint8_t band_of_bin[256];
    uint32_t blk_bits[6];           // bits of each block: nominal (from the bap codes) ...
    uint32_t blk_bits2[6];          // ... and as packed (a grouped code equal to the merged-marker takes none)
    int any_coll;
};

#ifndef ENC_PACKB_LB
#define ENC_PACKB_LB 4        // 128 VGPRs, 5 spilled, 24 bytes of scratch (6: 80 VGPRs, 204 bytes).  Its batches fit the chip several times over, so a frame's latency
                              // counts, not occupancy: cold encode 0.107 / 0.113 / 0.189 / 0.286 ms per 64 / 256 / 1 024 / 2 048 frames against 0.110 /
                              // 0.121 / 0.186 / 0.291 at 6
#endif
// MD (ac3mi_set_encode_metadata / _frames / _source, ac3mi_set_encode_drc): the BSI fields of P.bsi or of the frame's own word
// (pack_bsi), and the dynrng words of P.drc if it is set
// DW (with MD): compre / compr (compr2e / compr2) of P.compr, and the dynrng words of P.dyn - each programme's own - when it is
// set (enc_packf_kernel's DW)
template <bool MD = false, bool DW = false>
__global__ __launch_bounds__(384, ENC_PACKB_LB) void enc_packb_kernel(const PackParams P)
{
    static_assert(!DW || MD, "the array words are written where the profiles' are");
    __shared__ PackbLDS L;
    extern __shared__ uint4 pk_dyn[];
    uint32_t *fr = reinterpret_cast<uint32_t *>(pk_dyn);
    const int tid = threadIdx.x, lane = tid & 63;
    const int b = __builtin_amdgcn_readfirstlane(tid >> 6);
    PackbWave &W = L.w[b];
    // consecutive frames on one XCD (cdna_hip_programming.md T1): the six wavefronts' rows sit side by side in memory
    const size_t fidx = xcd_remap(blockIdx.x, gridDim.x);
    const int nch = P.nch, nfbw = P.nfbw, nbc = P.nbc, fs = P.frame_words;

    for (int i = tid; i < 256; i += 384) {
        L.band_of_bin[i] = P.tab->band_of_bin[i];
        L.crc_tab[i] = P.tab->crc_tab[i];
    }
    if (tid < 64) { const int bp = P.tab->baptab[tid]; L.packlut[tid] = mant_pack_entry(bp, plain_bits(bp)); }
    for (int i = tid; i < P.frw / 4; i += 384) reinterpret_cast<uint4 *>(fr)[i] = make_uint4(0, 0, 0, 0);
    const size_t rowb = (fidx * 6 + b) * nch;
    uint32_t mrows[3] = {0u, 0u, 0u};                   // the block's masking curves, two bands per dword (to LDS as band terms once the offsets are known)
    {
        const uint32_t *gm = reinterpret_cast<const uint32_t *>(P.emask + rowb * 50);
#pragma unroll
        for (int j = 0; j < 3; j++)
            if (lane + 64 * j < nch * 25) mrows[j] = gm[lane + 64 * j];
    }
    // lane = channel: exponent strategy and exp_samples of the block's channels
    const int strat_l = lane < nch ? (int)P.strat[rowb + lane] : 0;
    const int shift_l = lane < nch ? (int)P.shift[rowb + lane] : 0;
    uint32_t ew[6];                                     // the block's encoded exponents, four bins per lane and channel
#pragma unroll
    for (int ch = 0; ch < 6; ch++) ew[ch] = ch < nch ? *reinterpret_cast<const uint32_t *>(P.eexp + (rowb + ch) * 256 + 4 * lane) : 0u;
    int csnr, fsnr, snroffset;
    {
        const int w1 = P.snr[fidx * 2 + 1];
        csnr = P.snr[fidx * 2];
        fsnr = w1 & 15;
        snroffset = (((csnr - 15) << 4) + fsnr) << 2;
        if (w1 & 0x100) snroffset = (((w1 >> 9) - 15) << 4) << 2;      // a frame whose search failed: see enc_pack_kernel
    }
    if (tid == 0) L.any_coll = 0;
    mant_lists_init(W.glist, lane);
#pragma unroll
    for (int j = 0; j < 3; j++)
        if (lane + 64 * j < nch * 25) reinterpret_cast<uint32_t *>(&W.mask[0][0])[lane + 64 * j] = mant_band_terms(mrows[j], snroffset);
    const uint32_t bandoff = *reinterpret_cast<const uint32_t *>(&P.tab->band_of_bin[4 * lane]);
    __syncthreads();

    const uint32_t strat_lo = (uint32_t)__ballot(strat_l & 1), strat_hi = (uint32_t)__ballot(strat_l & 2);     // bit ch: the channel's strategy, bit 0 and 1
    auto strat_of = [&](int ch) { return ((strat_lo >> ch) & 1u) | (((strat_hi >> ch) & 1u) << 1); };
    // the frame's compr / compr2 words (DW), this block's dynrng words and its rematrixing word; then the bits of the frame header
    // (:1113-1147) and of this block's side information with its exponents (:1194-1332), i.e. where the blocks start:
    // enc_syntax.h's closed forms of the two field lists written below
    const bool dual = P.acmod == 0;
    const uint32_t compr0 = DW ? compr_word(P, fidx, 0) : 0u, compr1 = DW && dual ? compr_word(P, fidx, 1) : 0u;
    const uint32_t dynw0 = pack_dynrng<MD, DW>(P, fidx, b, 0), dynw1 = dual ? pack_dynrng<MD, DW>(P, fidx, b, 1) : 0u;
    const uint32_t rem = P.acmod == 2 && P.remat ? (uint32_t)P.remat[fidx * 6 + b] : b == 0 ? 0x10u : 0u;
    const SynShape shape{P.acmod, nfbw, nch, P.lfe != 0, dual, nbc, (uint32_t)P.chbwcod};
    const int hdr_bits = syn_header_bits(P.acmod, compr0, compr1), side_bits = syn_block_bits(shape, b, dynw0, dynw1, rem, strat_of);

    // the addresses of the block's coefficients into the bap table (:393-420), four per lane and channel
    uint32_t ad[6], em[6];
    int shv[6], neg;
#pragma unroll
    for (int ch = 0; ch < 6; ch++) shv[ch] = __builtin_amdgcn_readlane(shift_l, ch);
    mant_block_addresses(ad, em, neg, ew, shv, W.mask, bandoff, nch, nbc, P.lfe != 0, lane);
    const bool garbage = __ballot(neg < 0) != 0;

#pragma unroll 1
    for (int attempt = 0; attempt < 2; attempt++) {
        // ---- this block's bit count -> where it starts (second attempt: the counts as packed) ----
        int mant_bits = 0;
        if (attempt == 0) {
            uint32_t cnt = 0, plain = 0;            // kinds as 10-bit fields (<= 24 per lane), plain bits
#pragma unroll
            for (int ch = 0; ch < 6; ch++) {
                if (ch >= nch) continue;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint32_t w = L.packlut[(ad[ch] >> (8 * j)) & 63u].x;
                    cnt += 1u << (w >> 24);
                    plain += mant_pw_plain(w);
                }
            }
            const uint32_t s1 = wave_sum_u32((cnt & 1023u) | (((cnt >> 10) & 1023u) << 16));
            const uint32_t s2 = wave_sum_u32(((cnt >> 20) & 1023u) | (plain << 16));
            const int n1 = s1 & 0xffff, n2 = s1 >> 16, n4 = s2 & 0xffff;
            mant_bits = (int)(s2 >> 16) + 5 * ((n1 + 2) / 3) + 7 * ((n2 + 2) / 3) + 7 * ((n4 + 1) / 2);
            if (lane == 0) L.blk_bits[b] = (uint32_t)(side_bits + mant_bits);
        }
        __syncthreads();
        uint32_t pos = (uint32_t)hdr_bits;
        for (int q = 0; q < b; q++) pos += attempt == 0 ? L.blk_bits[q] : L.blk_bits2[q];

        // ---- side information (the frame header, from bit 0, is block 0's to write) ----
        if (b == 0) {
            PackSink k(fr, P.frw, lane, W.erow, [](int) { return 0u; }, 0, 0u);
            syn_header(k, P.fscod, P.frmsizecod, P.bsid, P.acmod, P.lfe != 0, dual, MD ? pack_bsi(P, fidx) : BSI_DEFAULT, compr0, compr1);
        }
        PackSink k(fr, P.frw, lane, W.erow, [&](int row) { return pick_row(ew, row, 0u); }, 0, pos);
        const uint8_t *bs = P.bsw ? P.bsw + rowb : nullptr;
        syn_block(k, shape, SynCpl{0u, 0, 12, 0u}, b, [&](int ch) -> uint32_t { return bs ? bs[ch] : 0u; },
                  [&](int p) { return p ? dynw1 : dynw0; }, rem, strat_of, [](int, int) { return 0u; }, (uint32_t)csnr, (uint32_t)fsnr);
        pos = k.pos;

        // ---- mantissas (:1341-1501): enc_mant.h ----
        {
            MantBlock B;
            B.fr = fr; B.frw = P.frw; B.glist = W.glist; B.packlut = L.packlut;
            B.mdb = P.mdct + rowb * 256;
            B.tap_bap = P.tap_bap ? P.tap_bap + rowb * 256 : nullptr;
            B.nch = nch; B.nbc = nbc; B.lfe = P.lfe != 0; B.marker = (uint32_t)P.marker;
            const uint32_t pos_m = pos;
            pos = mant_pack_block(B, em, ad, shv, garbage, pos, lane);
            // a grouped code that equals the merged-marker (:1466-1480) takes no bits: the block is shorter than its bap codes say,
            // i.e. every later block moves - the workgroup then packs the frame once more from the counts as packed
            if (attempt == 0 && lane == 0) {
                L.blk_bits2[b] = (uint32_t)side_bits + (pos - pos_m);
                if ((int)(pos - pos_m) != mant_bits) L.any_coll = 1;
            }
        }
        __syncthreads();
        if (attempt == 1 || !L.any_coll) break;
        __syncthreads();
        for (int i = tid; i < P.frw / 4; i += 384) reinterpret_cast<uint4 *>(fr)[i] = make_uint4(0, 0, 0, 0);
        __syncthreads();
    }

    // ---- frame end (:1599-1638): both CRC regions on one wavefront, then the frame goes out ----
    if (b == 0) {
        const uint32_t crcs = frame_crcs(L, fr, P, fs, lane);
        if (lane == 0) {
            fr[0] = (fr[0] & 0xffff0000u) | (crcs & 0xffff);                      // bytes 2,3
            const int p = 2 * fs - 2;                                                 // even -> inside one dword
            const int shft = 16 - 8 * (p & 3);
            fr[p >> 2] = (fr[p >> 2] & ~(0xffffu << shft)) | ((crcs >> 16) << shft);
        }
    }
    __syncthreads();
    uint8_t *dst = P.frames + fidx * P.frame_stride;
    for (int i = tid; i < (2 * fs + 3) / 4; i += 384) {
        const uint32_t v = __builtin_bswap32(fr[i]);
        const int rem = 2 * fs - 4 * i;
        if (rem >= 4) *reinterpret_cast<uint32_t *>(dst + 4 * i) = v;
        else for (int k = 0; k < rem; k++) dst[4 * i + k] = (uint8_t)(v >> (8 * k));
    }
}

#ifdef PACK_STAMPS
extern "C" __attribute__((visibility("default"))) int ac3mi_debug_pack_cycles(unsigned long long *out8, int reset)
{
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_pack_cycles), sizeof(unsigned long long) * 16) != hipSuccess) return -1;
    if (reset) { unsigned long long z[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_pack_cycles), z, sizeof z) != hipSuccess) return -1; }
    return 0;
}
#endif

// ---------------------------------------------------------------------------------------------
// Dynamic range control (ac3mi_set_encode_drc; the rule is include/ac3mi.h's).  Two kernels before the search:
//   enc_drc_gain_kernel    one wavefront per frame: the six block energies from the PCM (a read of its own: the DRC-off
//                          MDCT kernels stay as they are), levels relative to dialnorm and the profile's static gain
//   enc_drc_smooth_kernel  one lane per stream, its frames in order: the attack / release smoothing and the codes
// The tables are exact (no entry within 1e-4 of a rounding tie), computed once in double precision and frozen here:
//   DRC_LG[m] = round(256 log2(1 + m / 256)), DRC_XT[f] = round(32 (2^(f / 256) - 1)); DN[d] is folded in on the host, or, with a word per frame, picked by the frame's wavefront.
__constant__ uint8_t DRC_LG[256] = {
    0, 1, 3, 4, 6, 7, 9, 10, 11, 13, 14, 16, 17, 18, 20, 21, 22, 24, 25, 26, 28, 29, 30, 32, 33, 34, 36, 37, 38, 40, 41, 42,
    44, 45, 46, 47, 49, 50, 51, 52, 54, 55, 56, 57, 59, 60, 61, 62, 63, 65, 66, 67, 68, 69, 71, 72, 73, 74, 75, 77, 78, 79, 80, 81,
    82, 84, 85, 86, 87, 88, 89, 90, 92, 93, 94, 95, 96, 97, 98, 99, 100, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111, 112, 113, 114, 116, 117,
    118, 119, 120, 121, 122, 123, 124, 125, 126, 127, 128, 129, 130, 131, 132, 133, 134, 135, 136, 137, 138, 139, 140, 141, 142, 143, 144, 145, 146, 147, 148, 149,
    150, 151, 152, 153, 154, 155, 155, 156, 157, 158, 159, 160, 161, 162, 163, 164, 165, 166, 167, 168, 169, 169, 170, 171, 172, 173, 174, 175, 176, 177, 178, 178,
    179, 180, 181, 182, 183, 184, 185, 185, 186, 187, 188, 189, 190, 191, 192, 192, 193, 194, 195, 196, 197, 198, 198, 199, 200, 201, 202, 203, 203, 204, 205, 206,
    207, 208, 208, 209, 210, 211, 212, 212, 213, 214, 215, 216, 216, 217, 218, 219, 220, 220, 221, 222, 223, 224, 224, 225, 226, 227, 228, 228, 229, 230, 231, 231,
    232, 233, 234, 234, 235, 236, 237, 238, 238, 239, 240, 241, 241, 242, 243, 244, 244, 245, 246, 247, 247, 248, 249, 249, 250, 251, 252, 252, 253, 254, 255, 255};
__constant__ uint8_t DRC_XT[256] = {
    0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 3, 3, 3,
    3, 3, 3, 3, 3, 3, 3, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 6, 6, 6, 6, 6,
    6, 6, 6, 6, 6, 7, 7, 7, 7, 7, 7, 7, 7, 7, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 9, 9, 9, 9, 9, 9, 9, 9,
    9, 10, 10, 10, 10, 10, 10, 10, 10, 11, 11, 11, 11, 11, 11, 11, 11, 11, 12, 12, 12, 12, 12, 12, 12, 12, 13, 13, 13, 13, 13, 13,
    13, 13, 14, 14, 14, 14, 14, 14, 14, 14, 14, 15, 15, 15, 15, 15, 15, 15, 16, 16, 16, 16, 16, 16, 16, 16, 17, 17, 17, 17, 17, 17,
    17, 17, 18, 18, 18, 18, 18, 18, 18, 19, 19, 19, 19, 19, 19, 19, 20, 20, 20, 20, 20, 20, 20, 21, 21, 21, 21, 21, 21, 21, 22, 22,
    22, 22, 22, 22, 22, 23, 23, 23, 23, 23, 23, 23, 24, 24, 24, 24, 24, 24, 25, 25, 25, 25, 25, 25, 25, 26, 26, 26, 26, 26, 26, 27,
    27, 27, 27, 27, 27, 27, 28, 28, 28, 28, 28, 28, 29, 29, 29, 29, 29, 29, 30, 30, 30, 30, 30, 30, 31, 31, 31, 31, 31, 31, 32, 32};
// DN[d] = round(256 d / (20 log10 2)), d = dialnorm 0..31
static const int16_t DRC_DN[32] = {0, 43, 85, 128, 170, 213, 255, 298, 340, 383, 425, 468, 510, 553, 595, 638,
                                   680, 723, 765, 808, 850, 893, 935, 978, 1020, 1063, 1106, 1148, 1191, 1233, 1276, 1318};
// the static curves of profiles 1..5: MB, Rb, N0, N1, C0, Re, Rc (lv)
static const int16_t DRC_CURVE[5][7] = {{255, 2, 0, 213, 638, 2, 20}, {255, 2, -425, 425, 850, 2, 20}, {510, 2, 0, 213, 638, 2, 20},
                                        {510, 2, -425, 425, 425, 2, 2}, {638, 5, 0, 213, 638, 2, 20}};

struct DrcParams {
    const int16_t *pcm;         // [S][F][1536][nch] interleaved
    int16_t *gain;              // [S][F][6] static-curve gains (lv)
    uint8_t *code;              // [S][F][6] dynrng codes
    int32_t *state;             // [S] smoothing state (lv), or by slot
    const int32_t *slot;
    int n_streams, frames, nch;
    uint32_t fbw_in;            // bit c: input channel c is a coded full-bandwidth channel (chmap[0 .. nfbw - 1])
    int dn;                     // DN[dialnorm]
    const uint32_t *bsi_words;  // optional, [S][F]: frame f's level is relative to its own dialnorm, dn_tab[bsi_sanitise(bsi_words[f]) & 31]
    int16_t dn_tab[32];         // DN, for the frames' own picks (read from the kernel-argument segment)
    int mb, rb, n0, n1, c0, re, rc;
};

// VEC (the PCM 16-byte aligned, as every frame then is: 3 072 nch bytes apart): eight samples per load, a block's at most
// three loads per lane, all six blocks' in flight together; else one sample per load
template <bool VEC>
__global__ __launch_bounds__(64) void enc_drc_gain_kernel(const DrcParams Q)
{
    const int lane = threadIdx.x, nch = Q.nch, n = 256 * nch;
    const size_t fidx = blockIdx.x;
    const int16_t *fp = Q.pcm + fidx * 1536 * nch;
    uint64_t e6[6];
    if constexpr (VEC) {
        const uint4 *fv = reinterpret_cast<const uint4 *>(fp);
        const int nv = n / 8;                                   // 16-byte loads per block: 32 nch
        uint4 v[6][3];
#pragma unroll
        for (int b = 0; b < 6; b++)
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const int j = lane + 64 * k;
                v[b][k] = j < nv ? fv[b * nv + j] : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
        for (int b = 0; b < 6; b++) {
            uint64_t e = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const int j = lane + 64 * k;
                int c = (8 * j) % nch;                          // the channel of the load's first sample
                const uint32_t w[4] = {v[b][k].x, v[b][k].y, v[b][k].z, v[b][k].w};
#pragma unroll
                for (int t = 0; t < 8; t++) {
                    const int x = (int16_t)(w[t >> 1] >> (16 * (t & 1)));
                    if ((Q.fbw_in >> c) & 1u) e += (uint32_t)(x * x);
                    c = c + 1 == nch ? 0 : c + 1;
                }
            }
            e6[b] = e;
        }
    } else {
        const int c_first = lane % nch, c_step = 64 % nch;       // the channel of sample `lane` of a block, and its step per pass
#pragma unroll
        for (int b = 0; b < 6; b++) {
            const int16_t *bp = fp + (size_t)b * n;
            uint64_t e = 0;
            int c = c_first;
            for (int i = lane; i < n; i += 64) {
                const int x = bp[i];
                if ((Q.fbw_in >> c) & 1u) e += (uint32_t)(x * x);
                c += c_step;
                if (c >= nch) c -= nch;
            }
            e6[b] = e;
        }
    }
    const int dn = Q.bsi_words ? (int)Q.dn_tab[bsi_sanitise(Q.bsi_words[fidx]) & 31u] : Q.dn;
    int g_lane = 0;
#pragma unroll
    for (int b = 0; b < 6; b++) {
        uint64_t e = e6[b];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) e += __shfl_xor(e, o);
        // level (lv) relative to a full-scale sine on one channel, then to the dialogue level
        int lev = -4096;
        if (e) {
            const int k = 63 - __builtin_clzll(e);
            const int m = (int)(((e << 8) >> k) & 255u);
            lev = max(-4096, 256 * k + (int)DRC_LG[m] - 37 * 256);
        }
        const int r = lev + dn;
        int g;
        if (r < Q.n0) g = min(Q.mb, ((Q.n0 - r) * (Q.rb - 1)) / Q.rb);
        else if (r <= Q.n1) g = 0;
        else if (r <= Q.c0) g = -(((r - Q.n1) * (Q.re - 1)) / Q.re);
        else g = -(((Q.c0 - Q.n1) * (Q.re - 1)) / Q.re) - (((r - Q.c0) * (Q.rc - 1)) / Q.rc);
        g_lane = lane == b ? max(g, -1024) : g_lane;
    }
    if (lane < 6) Q.gain[fidx * 6 + lane] = (int16_t)g_lane;
}

__global__ __launch_bounds__(64) void enc_drc_smooth_kernel(const DrcParams Q)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= Q.n_streams) return;
    int32_t *sp = Q.state + (Q.slot ? Q.slot[s] : s);
    int st = *sp;
    for (int f = 0; f < Q.frames; f++) {
        const size_t fidx = (size_t)s * Q.frames + f;
        int16_t g6[6];
#pragma unroll
        for (int b = 0; b < 6; b++) g6[b] = Q.gain[fidx * 6 + b];
#pragma unroll
        for (int b = 0; b < 6; b++) {
            const long long d = (long long)g6[b] - st;          // (64 bits: a caller's state may be any int32)
            if (d < 0) st -= (int)max(1LL, (-d * 6631) >> 16);
            else if (d > 0) st += (int)max(1LL, (d * 349) >> 16);
            const int v = 32 * (st >> 8) + (int)DRC_XT[st & 255];
            Q.code[fidx * 6 + b] = (uint8_t)(v < -128 ? -128 : v > 127 ? 127 : v);
        }
    }
    *sp = st;
}

static hipError_t launch_drc(const EncodeLaunch &E, hipStream_t stream)
{
    const EncConfig &c = E.cfg;
    if (E.drc_profile < 1 || E.drc_profile > 5 || !E.drc_state || !E.ws_drc_gain || !E.ws_drc_code) return hipErrorInvalidValue;
    DrcParams Q;
    Q.pcm = E.pcm;
    Q.gain = E.ws_drc_gain;
    Q.code = E.ws_drc_code;
    Q.state = E.drc_state;
    Q.slot = E.slot;
    Q.n_streams = E.n_streams;
    Q.frames = E.frames_per_stream;
    Q.nch = c.nch;
    Q.fbw_in = 0;
    for (int ch = 0; ch < c.nfbw; ch++) Q.fbw_in |= 1u << E.chmap[ch];
    Q.dn = DRC_DN[E.bsi & 31u];
    Q.bsi_words = E.bsi_words;
    for (int d = 0; d < 32; d++) Q.dn_tab[d] = DRC_DN[d];
    const int16_t *k = DRC_CURVE[E.drc_profile - 1];
    Q.mb = k[0]; Q.rb = k[1]; Q.n0 = k[2]; Q.n1 = k[3]; Q.c0 = k[4]; Q.re = k[5]; Q.rc = k[6];
    const dim3 frames((unsigned)E.n_streams * (unsigned)E.frames_per_stream);
    if (((uintptr_t)E.pcm & 15) == 0) hipLaunchKernelGGL(enc_drc_gain_kernel<true>, frames, dim3(64), 0, stream, Q);
    else hipLaunchKernelGGL(enc_drc_gain_kernel<false>, frames, dim3(64), 0, stream, Q);
    hipLaunchKernelGGL(enc_drc_smooth_kernel, dim3((E.n_streams + 63) / 64), dim3(64), 0, stream, Q);
    return hipGetLastError();
}

// the kernels under the words of launch_rule.h's lists
template <uint32_t V> struct MdctVariant {
    static constexpr auto fn = enc_mdct_kernel<(V & V_BSW) != 0, (V & V_REMAT) != 0, (V & V_BW) != 0, (V & V_XS) != 0, (V & V_LFEROW) != 0, (V & V_FX) != 0>;
};
template <uint32_t V> struct CplVariant { static constexpr auto fn = enc_cpl_kernel<(V & V_BW) != 0, (V & V_XS) != 0, (V & V_R3) != 0>; };
template <uint32_t V> struct SearchVariant {
    static constexpr auto fn = enc_search_kernel<(int)(V & V_NUM), (V & V_CPL) != 0, (V & V_BW) != 0, (V & V_DRC) != 0, (V & V_FX) != 0, (V & V_DW) != 0>;
};
template <uint32_t V> struct PackfVariant {
    static constexpr auto fn = enc_packf_kernel<(V & V_FX) != 0, (V & V_CPL) != 0, (V & V_BW) != 0, (V & V_MD) != 0, (V & V_DUAL) != 0, (V & V_DW) != 0>;
};
template <uint32_t V> struct PackbVariant { static constexpr auto fn = enc_packb_kernel<(V & V_MD) != 0, (V & V_DW) != 0>; };
static_assert(ENC_MAX_COEFS == MANT_MAX_COEFS, "the rule's limit is the packers' member lists'");

// one stage of the rule's chain: the kernel under its word, on its grid (a stage that does not run: nothing)
template <const auto &LIST, template <uint32_t> class K, class Params>
static hipError_t launch_stage(const KernelLaunch &k, const EncodeLaunch &E, size_t lds, hipStream_t stream, const Params &P)
{
    if (k.family == K_NONE) return hipSuccess;
    const auto fn = variant_fn<LIST, K>(k.variant);
    if (!fn) return hipErrorInvalidValue;
    log_launch(E.log, k);
    hipLaunchKernelGGL(fn, dim3(grid_size(k, E.n_streams, E.frames_per_stream, E.cfg.nch)), dim3(k.block), lds, stream, P);
    return hipGetLastError();
}

// the chain of launch_rule.h's enc_choice: DRC kernels, (pre-pass,) front kernel, (LFE row, coupling, tabulation,) search,
// packer, (history)
hipError_t launch_encode(const DeviceTables &tab, const EncodeLaunch &E, hipStream_t stream)
{
    if (E.n_streams <= 0 || E.frames_per_stream <= 0) return hipSuccess;
    const EncConfig &c = E.cfg;
    const EncChoice R = enc_choice(E);
    if (R.err) return hipErrorInvalidValue;
    hipError_t e;
    if (R.drc && (e = launch_drc(E, stream)) != hipSuccess) return e;
    MdctParams M;
    M.pcm = E.pcm;
    M.last = E.last;
    M.mdct = E.ws_mdct;
    M.full_rows = E.mdct_full_rows ? 1 : 0;
    M.expo = E.ws_expo;
    M.shift = E.ws_shift;
    M.tab = tab.enc;
    M.n_streams = E.n_streams;
    M.frames = E.frames_per_stream;
    M.nch = c.nch;
    for (int i = 0; i < 8; i++) M.chmap[i] = E.chmap[i];
    M.slot = E.slot;
    M.store_history = !R.history;
    M.x.eexp = E.ws_eexp;
    M.x.emask = E.ws_emask;
    M.x.strat = E.ws_strat;
    M.x.ebits = E.ws_ebits;
    M.x.tab = tab.enc;
    M.x.nch = c.nch;
    M.x.lfe = c.lfe;
    M.x.fscod = c.fscod;
    M.x.halfrate = c.halfrate;
    M.x.nbc = R.nbc;    // the only reader of last[] is this same wavefront's block 0
    M.bsw = E.ws_bsw;
    M.remat = R.remat ? E.ws_remat : nullptr;
    if (R.stage[ES_PRE].family != K_NONE) {
        // coupling with rematrixing: the rows without rematrixing first (before the history is rewritten), for enc_cpl_kernel
        MdctParams M0 = M;
        M0.mdct = E.ws_cpl.prow;
        M0.shift = E.ws_cpl.pshift;
        M0.expo = nullptr;
        M0.full_rows = 1;
        M0.store_history = 0;
        M0.remat = nullptr;
        M0.x.eexp = E.ws_cpl.peexp;
        M0.x.emask = E.ws_cpl.pemask;
        M0.x.strat = E.ws_cpl.pstrat;
        M0.x.ebits = E.ws_cpl.pebits;
        if ((e = launch_stage<ENC_MDCT_VARIANTS, MdctVariant>(R.stage[ES_PRE], E, 0, stream, M0)) != hipSuccess) return e;
    }
    if ((e = launch_stage<ENC_MDCT_VARIANTS, MdctVariant>(R.stage[ES_MDCT], E, 0, stream, M)) != hipSuccess) return e;
    {
        MdctParams ML = M;                              // the LFE row beside the REMAT workgroups' two channels
        ML.remat = nullptr;
        if ((e = launch_stage<ENC_MDCT_VARIANTS, MdctVariant>(R.stage[ES_LFEROW], E, 0, stream, ML)) != hipSuccess) return e;
    }
    if (R.cpl) {
        CplParams C;
        C.mdct = E.ws_mdct;
        C.shift = E.ws_shift;
        C.bsw = E.ws_bsw;
        C.remat = M.remat;
        C.mdct_out = E.ws_mdct;
        C.shift_out = E.ws_shift;
        C.w = E.ws_cpl;
        C.x = M.x;
        C.x.nbc = 37 + 12 * E.cpl_begf;
        C.nfbw = c.nfbw;
        C.begf = E.cpl_begf;
        C.nfr = E.n_streams * E.frames_per_stream;
        C.endf = R.cpl_endf;
        C.nbc = R.nbc;
        if ((e = launch_stage<ENC_CPL_VARIANTS, CplVariant>(R.stage[ES_CPL], E, 0, stream, C)) != hipSuccess) return e;
    }

    PackParams P;
    P.mdct = E.ws_mdct;
    P.eexp = E.ws_eexp;
    P.emask = E.ws_emask;
    P.strat = E.ws_strat;
    P.ebits = E.ws_ebits;
    P.shift = E.ws_shift;
    P.csnr_state = E.csnr;
    P.slot = E.slot;
    P.frames = E.frames;
    P.tab = tab.enc;
    P.tap_eexp = E.tap_eexp;
    P.tap_bap = E.tap_bap;
    P.tap_strat = E.tap_strat;
    P.tap_snr = E.tap_snr;
    P.tap_curve = E.tap_curve;
    P.n_streams = E.n_streams;
    P.frames_per_stream = E.frames_per_stream;
    P.frame_stride = E.frame_stride;
    P.nch = c.nch;
    P.nfbw = c.nfbw;
    P.lfe = c.lfe;
    P.acmod = c.acmod;
    P.fscod = c.fscod;
    P.halfrate = c.halfrate;
    P.bsid = c.bsid;
    P.frmsizecod = c.frmsizecod;
    P.frame_words = c.frame_words;
    P.nbc = R.nbc;
    P.chbwcod = E.chbwcod;
    const int fs = c.frame_words;
    if (!E.crc_rows) return hipErrorInvalidValue;
    const CrcSplit split = crcl_split(fs);
    P.crc_rows = E.crc_rows;
    P.crc_c = split.C;
    P.crc_n1 = split.n1;
    P.snr = E.ws_snr;
    P.memo = R.memo ? E.ws_memo : nullptr;
    P.hint = E.search_hint;
    P.hint_stride = E.search_hint_stride;
    P.bsw = E.ws_bsw;
    P.remat = M.remat;
    P.cpl = R.cpl ? E.ws_cpl : CplWs{};
    P.cpl_begf = R.cpl ? E.cpl_begf : 0;
    P.cpl_endf = R.cpl_endf;
    P.drc = R.drc ? E.ws_drc_code : nullptr;
    P.bsi = E.bsi;
    P.bsi_words = E.bsi_words;
    P.dyn = E.dyn_codes;
    P.compr = E.compr_words;
#ifndef ENC_FR_HEADROOM
#define ENC_FR_HEADROOM 256
#endif
    P.frw = ((2 * fs + ENC_FR_HEADROOM + 15) / 16) * 4;
    P.marker = getenv("AC3MI_ENC_MARKER") ? atoi(getenv("AC3MI_ENC_MARKER")) : 128;      // test aid (read per launch), see PackParams::marker
    static const int lds_pad = getenv("AC3MI_ENC_LDS_PAD") ? atoi(getenv("AC3MI_ENC_LDS_PAD")) : 0;      // profiling aid: occupancy sweeps
    const size_t fr_lds = (size_t)P.frw * 4 + lds_pad;
    if ((e = launch_stage<ENC_SEARCH_VARIANTS, SearchVariant>(R.stage[ES_TABULATE], E, 0, stream, P)) != hipSuccess) return e;
    if ((e = launch_stage<ENC_SEARCH_VARIANTS, SearchVariant>(R.stage[ES_SEARCH], E, 0, stream, P)) != hipSuccess) return e;
    e = R.packb ? launch_stage<ENC_PACKB_VARIANTS, PackbVariant>(R.stage[ES_PACK], E, fr_lds, stream, P)
                : launch_stage<ENC_PACKF_VARIANTS, PackfVariant>(R.stage[ES_PACK], E, fr_lds, stream, P);
    if (e != hipSuccess) return e;
    // the new history: last 256 samples per channel of each stream's final frame
    return R.history ? launch_enc_history(E, stream) : hipSuccess;
}

__global__ void enc_history_kernel(const int16_t *pcm, int16_t *last, int n_streams, int frames, int nch, const uint8_t c0,
                                   const uint8_t c1, const uint8_t c2, const uint8_t c3, const uint8_t c4, const uint8_t c5,
                                   const int32_t *slot)
{
    const uint8_t chmap[6] = {c0, c1, c2, c3, c4, c5};
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;          // (s*nch + ch)*256 + j
    if (idx >= n_streams * nch * 256) return;
    const int j = idx & 255, ch = (idx >> 8) % nch, s = (idx >> 8) / nch;
    const int16_t *fp = pcm + ((size_t)s * frames + (frames - 1)) * 1536 * nch;
    const int16_t v = fp[(size_t)(5 * 256 + j) * nch + chmap[ch]];
    if (slot) last[((size_t)slot[s] * 6 + ch) * 256 + j] = v;
    else last[idx] = v;
}

CplWs cpl_slices(void *base, size_t nfr)
{
    uint8_t *p = (uint8_t *)base;
    CplWs w;
    auto take = [&](size_t n) { uint8_t *q = p; p += (n + 15) & ~(size_t)15; return q; };
    w.word = (uint32_t *)take(4 * nfr);
    w.co = take(80 * nfr);
    w.mdct = (int32_t *)take(6 * 256 * 4 * nfr);
    w.shift = (int8_t *)take(8 * nfr);
    w.eexp = take(6 * 256 * nfr);
    w.emask = (int16_t *)take(6 * 50 * 2 * nfr);
    w.strat = take(8 * nfr);
    w.ebits = (int32_t *)take(4 * nfr);
    return w;
}

void cpl_remat_slices(CplWs &w, void *base, size_t nfr, int nrow)
{
    uint8_t *p = (uint8_t *)base;
    auto take = [&](size_t n) { uint8_t *q = p; p += (n + 15) & ~(size_t)15; return q; };
    const size_t r16 = (size_t)((6 * nrow + 15) & ~15), e16 = (size_t)((4 * nrow + 15) & ~15);   // (cpl_remat_frame_bytes)
    w.prow = (int32_t *)take(6 * nrow * 256 * 4 * nfr);
    w.pshift = (int8_t *)take(r16 * nfr);
    w.peexp = take(6 * nrow * 256 * nfr);
    w.pemask = (int16_t *)take(6 * nrow * 50 * 2 * nfr);
    w.pstrat = take(r16 * nfr);
    w.pebits = (int32_t *)take(e16 * nfr);
}

hipError_t launch_enc_history(const EncodeLaunch &E, hipStream_t stream)
{
    const int n = E.n_streams * E.cfg.nch * 256;
    hipLaunchKernelGGL(enc_history_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, E.pcm, E.last, E.n_streams,
                       E.frames_per_stream, E.cfg.nch, E.chmap[0], E.chmap[1], E.chmap[2], E.chmap[3], E.chmap[4], E.chmap[5], E.slot);
    return hipGetLastError();
}

}  // namespace ac3mi
