// decode_kernel.h — decode_kernel<MODE, FX, SRC>, the front end of decode.hip (see there), as a header: decode.hip instantiates
// it, and decode_src.hip instantiates the one variant that must not share a translation unit with its twin.
// Which heads it refuses and a frame's own size: frame_own_bytes (decode_common.h) on sync_rule.h, as the workgroup kernel.
// The side information it reads: the field lists of dec_syntax.h, as the workgroup kernel; its own are the reader (Rd), the state
// (St) and the sink (DkSink), and everything computed from what was read.
#pragma once
#include "decode_common.h"
#include "mant2.h"

namespace ac3mi {

// ---------------------------------------------------------------------------

// MODE 0: one wavefront per stream, frames in order (the dither LFSR carries from frame to frame), everything in one
// kernel: the front end of rounds 1-2, kept as the bit-identity reference of the tests and for A/B runs (ac3mi_set_decode_mode 1).
// Nothing else carries across the frames of a valid stream (block 0 re-sends exponents, coupling and bit-allocation
// parameters): the frame-parallel variant below (MODE 5) rests on that.
// Wavefronts per SIMD the register budget is set for.  MODE 0 runs as fast with 4 (128 VGPRs, 52 B of scratch) as with 5
// (96 VGPRs, 160 B of scratch) on one-frame streams and 9 % faster on 8-frame streams, and leaves a third of the spill traffic.
#ifndef DEC_LB0
#define DEC_LB0 4
#endif
// MODE 4 (one wavefront per stream) / MODE 5 + lfsr_prefix_kernel (one per frame): the parse half of the split front
// end - side information, exponents, bit allocation; the mantissas of a block are only COUNTED, from per-row totals, and
// mant_kernel (one wavefront per audio block, a workgroup per frame) unpacks them from the block descriptors and rows
// this kernel leaves in the workspace (BlkDesc, mant2.h).
#ifndef DEC_LBP
#define DEC_LBP 5
#endif
// Measurement aid (make EXTRA=-DDEC_STAMPS, a separate library): lane 0 of every wavefront adds the s_memtime cycles of
// a frame's sections to g_dec_cycles: 0 staging + header, 1 side information, 2 exponents, 3 bit-allocation parameters +
// bit allocation, 4 mantissas (+ coupling, rematrix, stores), 5 the rest.  ac3mi_debug_dec_cycles reads them.
#ifdef DEC_STAMPS
__device__ unsigned long long g_dec_cycles[8];
#define DK_DECL() unsigned long long dk_t = 0, dk_acc[6] = {0, 0, 0, 0, 0, 0}
#define DK_T0() dk_t = __builtin_readcyclecounter()
#define DK_LAP(id) do { const unsigned long long t_ = __builtin_readcyclecounter(); dk_acc[id] += t_ - dk_t; dk_t = t_; } while (0)
#define DK_END() do { if (lane == 0) for (int i_ = 0; i_ < 6; i_++) atomicAdd(&g_dec_cycles[i_], dk_acc[i_]); } while (0)
#define DK_SINK , dk_t, dk_acc
#else
#define DK_DECL() do { } while (0)
#define DK_T0() do { } while (0)
#define DK_LAP(id) do { } while (0)
#define DK_END() do { } while (0)
#define DK_SINK
#endif

// decode_kernel's sink of the field lists (dec_syntax.h): coupling coordinates and deltba rows into the wavefront's LDS, the
// exponent groups read where they stand, dynamic-range words through the call's taps; SRC: the block's raw words collect in raw
template <bool SRC>
struct DkSink {
    DecLDS &L;
    const DecodeParams &P;
    const FrameBits FB;
    size_t blk_index;                   // fidx * 6 + blk
    int lane;
    uint32_t raw;
#ifdef DEC_STAMPS
    unsigned long long &dk_t, *dk_acc;
#endif
    __device__ __forceinline__ float dynrng(int code, int word, bool apply)
    {
        if constexpr (SRC) raw |= src_dyn_field(code, word);
        return apply ? dynrng_range(P, code, blk_index * 2 + word, lane) : 0.f;
    }
    __device__ __forceinline__ void cplco(int ch, int bnd, int ex, int ma, int master)
    {
        const float co = cplco_value(ex, ma, master);
        if (lane == 0) L.cplco[ch][bnd] = co;
    }
    __device__ __forceinline__ void cplco_flip(int bnd) { if (lane == 0) L.cplco[1][bnd] = -L.cplco[1][bnd]; }
    __device__ __forceinline__ int exponents(int slot, int es, int ngrp, int e0, int start, uint32_t pos)
    {
        uint8_t *row = L.exp + row_off(slot);
        if (slot != 6 && lane == 0) row[0] = (uint8_t)e0;
        return read_exponents(FB, pos, es, ngrp, e0, row + (slot == 6 ? start : 1), lane);
    }
    __device__ __forceinline__ void deltba_clear(int slot) { if (lane < 50) L.deltba[slot][lane] = 0; }
    __device__ __forceinline__ void deltba_seg(int slot, int band, int len, int d) { if (lane < len) L.deltba[slot][band + lane] = (int8_t)d; }
    __device__ __forceinline__ void lap(int point) { if (point == 2) DK_LAP(1); }
};

// (crc_verdicts() reads DecodeParams::crc from the kernel-argument segment: P must stay this kernel's first argument)
// FX (MODE 4; launch_decode's fixed-shape rule): one-frame 5.1 streams - a single frame (no frame loop, nothing carried from
// frame to frame), acmod 7 with the LFE, five full-bandwidth channels, six planes and no stage taps as constants.  A frame
// whose header says otherwise is refused by the same tests, and its blocks then run none of the code that uses them.
// SRC (ac3mi_set_encode_drc_source 1, a transcode's front end; never with FX): every block that is read leaves its raw dynrnge /
// dynrng (dynrng2e / dynrng2) fields in P.src_dyn, whether or not the decode applies them, for enc_dynrng_source_kernel
template <int MODE, bool FX = false, bool SRC = false>
__global__ __launch_bounds__(64, MODE >= 4 ? DEC_LBP : DEC_LB0) void decode_kernel(const DecodeParams P)
{
    static_assert(!(FX && SRC), "a call in source mode takes the generic kernels");
    static_assert(MODE == 0 || MODE == 4 || MODE == 5, "the one-kernel front ends per frame (1, 2) were retired in round 4");
    constexpr bool SERIAL = MODE == 0 || MODE == 4;         // one wavefront per stream, frames in order
    static_assert(!FX || MODE == 4, "the fixed 5.1 shape is the per-stream parse kernel's");
    constexpr bool PARSE = MODE >= 4;                       // no mantissa values: block descriptors + rows for mant_kernel
    __shared__ DecLDS L;
    extern __shared__ uint32_t frw[];
    const FrameBits FB{frw, (uint32_t)((P.frame_bytes + 3) >> 2) + 2u};
    const int lane = threadIdx.x;
    const int s = SERIAL ? (int)blockIdx.x : (int)(blockIdx.x / (unsigned)P.frames_per_stream);
    const int f_first = SERIAL ? 0 : (int)(blockIdx.x - (unsigned)s * (unsigned)P.frames_per_stream);
    const int f_end = SERIAL ? (FX ? 1 : P.frames_per_stream) : f_first + 1;
    const int n_in = FX ? 6 : P.n_in, nfchans = FX ? 5 : P.nfchans;
    if (s >= P.n_streams) return;

    // ---- constant tables into LDS ----
    for (int i = lane; i < 256; i += 64) L.la_neg[i] = P.tab->la_neg[i];
    if (lane < 50) L.hth[lane] = 0;
    L.width[lane] = remap_width(P.tab->width[lane]);        // row bytes: see decode_common.h, mantissa stage
    for (int i = lane; i < 100; i += 64) L.desc[i] = mant_desc((uint32_t)i);
    if (lane < 30) L.band_end[lane] = P.tab->band_end[lane];
    for (int i = lane; i < 256; i += 64) L.band_of_bin[i] = P.tab->band_of_bin[i];
    {
        // exp, bap, deltba and cplco are adjacent and dword-sized together: zeroed as dwords (a byte loop took 26 rounds)
        static_assert(offsetof(DecLDS, exp) == 0 && offsetof(DecLDS, bap) == ROWS && offsetof(DecLDS, deltba) == 2 * ROWS &&
                      offsetof(DecLDS, cplco) == 2 * ROWS + 6 * 52 && offsetof(DecLDS, gcode) == 2 * ROWS + 6 * 52 + 90 * 4 && ROWS % 4 == 0, "layout");
        uint32_t *z = reinterpret_cast<uint32_t *>(&L);
        for (int i = lane; i < (2 * ROWS + 6 * 52 + 90 * 4) / 4; i += 64) z[i] = 0u;
    }

    wave_sync();
    int ba_lo0, ba_hi0;                 // the lane's wide band (ba_wide_psd)
    ba_lane_band(L, lane, ba_lo0, ba_hi0);

    St st;
    const int sslot = P.slot ? P.slot[s] : s;
    DK_DECL();
    st.lfsr = (MODE == 0 || MODE == 4) ? (uint32_t)P.lfsr_state[sslot] : 1u;
    int hth_fscod = -1;
    uint32_t frame_draws = 0;
    // MODE 4: the generator's position along its cycle instead of its state (k draws = k positions)
    const bool pos_live = st.lfsr != 0;
    uint32_t lfsr_pos = MODE == 4 ? (uint32_t)P.lfsr_idx[st.lfsr] : 0u;
    if (PARSE && lane < 7) L.tot[lane][2] = 0;

    for (int f = f_first; f < f_end; f++) {
        const size_t fidx = FX ? (size_t)s : (size_t)s * P.frames_per_stream + f;
        const uint8_t *src = P.frames + fidx * P.frame_stride;
        float *cout = P.coef + fidx * 6 * n_in * 256;
        uint32_t status = 0;
        [[maybe_unused]] int short_bytes = 0;       // the frame's own size where it is below frame_bytes (BlkDesc::own_bytes), else 0
        // block 0 takes exponents, coupling or bit-allocation parameters the frame did not send (not a conforming frame):
        // what it reuses is whatever the variant at hand has carried so far, so results may depend on the batch shape
        bool reuse0 = false;
        // parse modes: rows of this frame's row sets not written yet (bit = slot), and the block that holds each slot's
        // current row (4 bits per slot)
        int dirty_exp = 0x7f, dirty_bap = 0x7f;
        uint32_t rv_exp = 0, rv_bap = 0;            // lane = slot
        if (MODE == 4) frame_draws = 0;

        DK_T0();
        // ---- stage the frame: byte-swapped dwords, zero padded ----
        {
            const int nw = (P.frame_bytes + 3) >> 2;
            const uint32_t *s32 = reinterpret_cast<const uint32_t *>(src);
            // (the mantissa stage reads three dwords from index <= nw + 2.)  Eight loads in flight per lane before the first
            // is used: a 1536-byte frame is one round instead of seven dependent ones
            for (int base = 0; base < nw + 6; base += 512) {
                uint32_t v[8];
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int i = base + lane + 64 * k;
                    v[k] = i < nw ? s32[i] : 0u;
                }
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int i = base + lane + 64 * k;
                    const int rem = P.frame_bytes - 4 * i;
                    uint32_t x = v[k];
                    if (rem < 4 && rem > 0) x &= (1u << (8 * rem)) - 1u;
                    if (i < nw + 6) frw[i] = __builtin_bswap32(x);
                }
            }
        }
        wave_sync();

        Rd rd{FB, 0, 0, 0};
        // ---- a52_syncinfo (the header rule: sync_rule.h through frame_own_bytes) + a52_frame (dsyn_frame, dec_syntax.h) ----
        bool hdr_ok = true;
        if (const uint8_t *crcp = crc_verdicts())           // ac3mi_set_decode_crc 2: the CRC kernel's verdict (wave-uniform) refuses the frame
            if (crcp[fidx] & 0x40u) hdr_ok = false;
        {
            const uint32_t w0 = rfl(frw[0]), w1 = rfl(frw[1]);
            const int own = frame_own_bytes(w0, w1, P.frame_bytes);
            if (!own) hdr_ok = false;
            if (hdr_ok) {
                st.set_fscod(w1 >> 30);                            // w1 = bytes 4-7: fscod | frmsizecod, bsid | bsmod, acmod | ...
                st.set_halfrate(sync_halfrate((w1 >> 19) & 31));
                st.acmod = (w1 >> 13) & 7;
                if (st.acmod != (FX ? 7 : P.acmod)) hdr_ok = false;
                if (own < P.frame_bytes) {                         // (wave-uniform) the slot's bytes behind a shorter frame are not the frame's
                    trim_staged_frame(frw, own, (P.frame_bytes + 3) >> 2, lane, 64);
                    short_bytes = own;
                    wave_sync();
                }
            }
        }
        if (hdr_ok) {
            rd.seek(6 * 8 + 3);
            const DsynRequest q{FX ? 1 : P.lfeon, P.req_flags, P.level, P.dynrng_on ? 1 : 0};
            const int output = dsyn_frame(rd, st, FX ? 7 : st.acmod, q);
            hdr_ok = output >= 0;
            if (hdr_ok) {
                if (hth_fscod != st.fscod()) {
                    if (lane < 50) L.hth[lane] = P.tab->hth[st.fscod()][lane];
                    hth_fscod = st.fscod();
                }
                status |= (uint32_t)output << 16;
            }
        }
        if (!hdr_ok) status |= 0x100u | 0x3fu;

        bool frame_dead = !hdr_ok;
        // (the blocks of a frame that passed the header test: its acmod and lfeon are the call's)
        const int acm = FX ? 7 : st.acmod, lfeon = FX ? 1 : st.lfeon();
        DK_LAP(0);
        for (int blk = 0; blk < 6; blk++) {
            float *cblk = cout + (size_t)blk * n_in * 256;
            const int in_lfe = FX ? 1 : P.lfeon ? 1 : 0;
            int err = frame_dead ? 1 : 0;
            DsynBlock sd{};                         // blksw / dithflag masks, strategies, the slots to allocate anew
            bool bd_ok = false;
            float gain[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
            const int nf = FX ? 5 : st.nf();

            if (!err) do {
                // ---- side information and exponents: the field lists of dec_syntax.h ----
                DkSink<SRC> k{L, P, FB, fidx * 6 + blk, lane, 0u DK_SINK};
                err = dsyn_block_a(rd, st, k, sd, blk, acm, nf, lfeon);
                if constexpr (SRC) if (lane == 0) P.src_dyn[fidx * 6 + blk] = k.raw;
                if (sd.reuse0) reuse0 = true;
                if (err) break;
                DK_LAP(2);
                dirty_exp |= sd.redo;                                       // (bits: 0..4 fbw, 5 lfe, 6 coupling channel)
                err = dsyn_block_b(rd, st, k, sd, blk, nf, lfeon);
                if (sd.reuse0) reuse0 = true;
                if (err) break;
                const int redo = sd.redo;
                wave_sync();

                // ---- bit allocation: parse.c:774-798 ----
                if (redo) {
                    bool allzero = !st.csnroffst() && !(st.chincpl() && (st.cbai(6) >> 3)) && !(lfeon && (st.cbai(5) >> 3));
#pragma unroll
                    for (int i = 0; i < 5; i++)
                        if (i < nf && (st.cbai(i) >> 3)) allzero = false;
                    dirty_bap |= allzero ? 0x7f : redo;
                    if (PARSE && lane < 7 && (allzero || ((redo >> lane) & 1))) L.tot[lane][2] = 0;
                    if (allzero) {
                        for (int i = lane; i < ROWS; i += 64) L.bap[i] = 0;
                    } else {
                        // the channel slots that need a new allocation, two per sweep of the band PSDs (wave-uniform; written
                        // out rather than as lambdas over `st`: a closure that holds its address keeps the whole state in scratch)
#define AC3MI_SLOT_END(slot) st.endm(slot)
                        int todo = redo & (((1 << nf) - 1) | (lfeon ? 32 : 0) | (st.chincpl() ? 64 : 0));
#pragma unroll
                        for (int i = 0; i < 5; i++) if (st.endm(i) <= 0) todo &= ~(1 << i);
                        if (st.cplendmant() <= st.cplstrtmant()) todo &= ~64;
                        while (todo) {
                            const int sA = __builtin_ctz(todo);
                            todo &= todo - 1;
                            const bool two = todo != 0;
                            const int sB = two ? __builtin_ctz(todo) : sA;
                            if (two) todo &= todo - 1;
                            const int stA = sA == 6 ? st.cplstrtmant() : 0, stB = sB == 6 ? st.cplstrtmant() : 0;
                            const int enA = AC3MI_SLOT_END(sA), enB = AC3MI_SLOT_END(sB);
                            const int wide = ba_wide_psd(L, ba_lo0, ba_hi0, L.exp + row_off(sA), stA, enA, L.exp + row_off(sB), stB, enB, two, lane);
                            for (int h = 0; h < (two ? 2 : 1); h++) {          // (one call site: the routine is inlined once)
                                const int slot = h ? sB : sA, start = h ? stB : stA, end = h ? enB : enA;
                                const int mybai = st.cbai(slot);
                                const int mydeltbae = slot == 5 ? 2 : st.deltbae(slot == 6 ? 5 : slot);
                                const BaCtx c = ba_ctx(st.bai(), mybai, st.csnroffst(), st.halfrate(), L.hth,
                                                       mydeltbae == 2 ? nullptr : L.deltba[slot == 6 ? 5 : slot],
                                                       slot == 6 ? st.cplfleak() << 8 : 0, slot == 6 ? st.cplsleak() << 8 : 0);
                                bit_allocate_finish(L, L.bmask, c, slot == 6 ? st.cplstrtbnd() : 0, start, end, L.exp + row_off(slot), L.bap + row_off(slot), wide, h, lane);
                            }
                        }
#undef AC3MI_SLOT_END
                    }
                    wave_sync();
                }
                dsyn_skip_field(rd);
            } while (0);
            const int blkswm = sd.blkswm, dithmask = sd.dithmask;

            // optional stage taps
            if (!FX && P.tap_exp) {
                uint8_t *te = P.tap_exp + (fidx * 6 + blk) * 7 * 256;
                int8_t *tb = P.tap_bap + (fidx * 6 + blk) * 7 * 256;
                for (int c = 0; c < 7; c++)
                    for (int i = lane; i < 256; i += 64) {
                        const bool in = c != 5 || i < LFE_ROW;
                        te[c * 256 + i] = in ? L.exp[row_off(c) + i] : 0;
                        tb[c * 256 + i] = in ? unmap_width(L.bap[row_off(c) + i]) : 0;
                    }
            }

            if (!err) {
                DK_LAP(3);
                // ---- gains: parse.c:810-811 ----
                a52_downmix_coeff_hd(gain, acm, st.output(), st.dynrng(), st.clev(), st.slev());

                // ---- mantissas: the segments of the block in bitstream order (mant_block, decode_common.h) ----
                if (!PARSE && st.chincpl() && lane < 18) {                    // sub-band -> band (parse.c:448-456)
                    const uint32_t below = st.cplbndstrc() & ((1u << lane) - 1u);
                    L.cplbnd[lane] = (uint8_t)(lane - __popc(below));
                }
                SegBase sb;
                sb.bit = rd.pos();
                sb.r3 = sb.r5 = sb.r11 = sb.draw = 0;
                if constexpr (!PARSE) {
                    MantBlk B;
                    B.nf = nf; B.lfeon = lfeon; B.acmod = acm; B.in_lfe = in_lfe;
                    B.chincpl = st.chincpl(); B.dithmask = dithmask; B.rematflg = st.rematflg();
                    B.cplstrtmant = st.cplstrtmant(); B.cplendmant = st.cplendmant();
#pragma unroll
                    for (int i = 0; i < 5; i++) { B.endmant[i] = st.endm(i); B.gain[i] = gain[i]; }
                    B.lfe_gain = (st.output() & AC3MI_LFE) ? st.dynrng() : 0.f;
                    const uint32_t lfsr_i0 = P.lfsr_idx[st.lfsr];
                    const bool lfsr_live = st.lfsr != 0;
                    mant_block<false>(B, [&](int slot) { return (const uint8_t *)L.exp + row_off(slot); },
                                          [&](int slot) { return (const int8_t *)L.bap + row_off(slot); },
                                          [&](int c, int bnd) { return L.cplco[c][bnd]; }, L.cplbnd, L.desc, L.gcode, frw, FB.last,
                                          P.tab->qtab, P.lfsr_seq, lfsr_i0, lfsr_live, cblk, sb, lane);
                    // advance the dither generator past this block's draws
                    if (lfsr_live && sb.draw) st.lfsr = P.lfsr_seq[(lfsr_i0 + (uint32_t)sb.draw) % 65535u];
                } else {
                    // parse only: the totals of every segment's row (cached per slot while row and range stay) give the bits and
                    // the dither draws of the block; rows that changed go to the workspace; the descriptor names them.
                    // Lane k takes segment k (the scalar unit is this kernel's bottleneck: a loop over the segments on
                    // wave-uniform values costs 600 scalar instructions per block, this form about 80 vector ones).
                    const int cplfirst = st.chincpl() ? __builtin_ctz(st.chincpl()) : 99;
                    const int nseg = nf + (st.chincpl() ? 1 : 0) + (lfeon ? 1 : 0);
                    const int ncpl_dith = __popc(st.chincpl() & dithmask);
                    const int k = lane;
                    const int slot_l = st.chincpl() ? (k <= cplfirst ? k : k == cplfirst + 1 ? 6 : k - 1 < nf ? k - 1 : 5) : (k < nf ? k : 5);
                    const bool seg_l = k < nseg;
                    const int end_l = st.endm(slot_l);
                    const int start_l = slot_l == 6 ? st.cplstrtmant() : 0;
                    const int mult_l = slot_l < 5 ? (dithmask >> slot_l) & 1 : slot_l == 6 ? ncpl_dith : 0;
                    const uint32_t key_l = 0x80000000u | (uint32_t)start_l | ((uint32_t)end_l << 10);
                    uint32_t ca = L.tot[slot_l][0], cb = L.tot[slot_l][1];
                    for (unsigned long long miss = __ballot(seg_l && L.tot[slot_l][2] != key_l); miss; miss &= miss - 1) {
                        const int k0 = __builtin_ctzll(miss);
                        const int s0 = __builtin_amdgcn_readlane(slot_l, k0);
                        const RowTotals T = row_totals(L.bap + row_off(s0), __builtin_amdgcn_readlane(start_l, k0), __builtin_amdgcn_readlane(end_l, k0),
                                                       s0 == 5 ? LFE_ROW / 4 : 64, lane);
                        if (lane == k0) { ca = T.a; cb = T.b; L.tot[s0][0] = T.a; L.tot[s0][1] = T.b; L.tot[s0][2] = key_l; }
                    }
                    {
                        const uint32_t n3 = seg_l ? (ca >> 13) & 511u : 0u, n5 = seg_l ? ca >> 22 : 0u, n11 = seg_l ? cb & 511u : 0u;
                        const uint32_t nz = seg_l ? cb >> 9 : 0u, plain = seg_l ? ca & 0x1fffu : 0u;
                        // 3/5/11-level members of the block before the segment
                        const uint32_t own35 = n3 | (n5 << 16), p35 = wave_incl_scan_u32(own35) - own35, r11 = wave_incl_scan_u32(n11) - n11;
                        const uint32_t r3 = p35 & 0xffffu, r5 = p35 >> 16;
                        // a grouped code takes its bits where the member of rank 0 mod 3 (mod 2) stands
                        auto div3 = [](uint32_t x) { return (x * 0xaaabu) >> 17; };
                        const uint32_t o3 = div3(r3 + n3 + 2u) - div3(r3 + 2u), o5 = div3(r5 + n5 + 2u) - div3(r5 + 2u);
                        const uint32_t o11 = ((r11 + n11 + 1u) >> 1) - ((r11 + 1u) >> 1);
                        const uint32_t bits_l = plain + 5u * o3 + 7u * (o5 + o11);
                        const uint32_t tot = wave_sum_u32(bits_l | ((nz * (uint32_t)mult_l) << 16));
                        sb.bit += tot & 0xffffu;
                        sb.draw = (int)(tot >> 16);
                    }
                    {
                        uint8_t *rowset = P.rows + (fidx * 6 + blk) * (size_t)ROWSET;
                        const int used = ((1 << nf) - 1) | (lfeon ? 32 : 0) | (st.chincpl() ? 64 : 0);
                        const int we = dirty_exp & used, wb = dirty_bap & used;
                        for (int m = we; m; m &= m - 1) {
                            const int s0 = __builtin_ctz(m);
                            if (lane < (s0 == 5 ? LFE_ROW / 4 : 64))
                                *reinterpret_cast<uint32_t *>(rowset + s0 * 512 + 4 * lane) = *reinterpret_cast<const uint32_t *>(L.exp + row_off(s0) + 4 * lane);
                        }
                        for (int m = wb; m; m &= m - 1) {
                            const int s0 = __builtin_ctz(m);
                            if (lane < (s0 == 5 ? LFE_ROW / 4 : 64))
                                *reinterpret_cast<uint32_t *>(rowset + s0 * 512 + 256 + 4 * lane) = *reinterpret_cast<const uint32_t *>(L.bap + row_off(s0) + 4 * lane);
                        }
                        dirty_exp &= ~we;
                        dirty_bap &= ~wb;
                        // lane = slot: the block of this frame that holds the slot's current rows
                        rv_exp = ((we >> lane) & 1) ? (uint32_t)blk : rv_exp;
                        rv_bap = ((wb >> lane) & 1) ? (uint32_t)blk : rv_bap;
                    }
                    if (st.chincpl()) {
                        float *cc = P.cplco + (fidx * 6 + blk) * 90;
                        cc[lane] = (&L.cplco[0][0])[lane];
                        if (lane < 26) cc[64 + lane] = (&L.cplco[0][0])[64 + lane];
                    }
                    // the descriptor, straight from the lanes, one lane per field: lanes 0-3 the first four dwords, 0-7 the eight
                    // halfwords from endmant on and the row indices, 0-6 the seven dwords from gain on (BlkDesc, mant2.h,
                    // asserts that the members lie so)
                    {
                        uint8_t *dp = reinterpret_cast<uint8_t *>(P.desc + (fidx * 6 + blk));
                        const uint32_t fl = ((uint32_t)st.chincpl() << BLK_CHINCPL) | ((uint32_t)dithmask << BLK_DITH) | ((uint32_t)st.rematflg() << BLK_REMAT);
                        const uint32_t w0 = lane == 0 ? rd.pos() : lane == 1 ? frame_draws : lane == 2 ? fl : st.cplbndstrc();
                        if (lane < 4) reinterpret_cast<uint32_t *>(dp)[lane] = w0;
                        const int em = lane == 5 ? st.cplstrtmant() : lane == 7 ? short_bytes : st.endm(lane & 7);
                        if (lane < 8) reinterpret_cast<uint16_t *>(dp + offsetof(BlkDesc, endmant))[lane] = (uint16_t)em;
                        if (lane < 8) { dp[offsetof(BlkDesc, rv_exp) + lane] = (uint8_t)rv_exp; dp[offsetof(BlkDesc, rv_bap) + lane] = (uint8_t)rv_bap; }
                        const float gl = lane == 0 ? gain[0] : lane == 1 ? gain[1] : lane == 2 ? gain[2] : lane == 3 ? gain[3] : lane == 4 ? gain[4]
                                       : (st.output() & AC3MI_LFE) ? st.dynrng() : 0.f;
                        // src_snr: the frame's own SNR offsets, 16 csnroffst + fsnroffst of channel 0 - a transcode's encoder starts
                        // costing its search there (a hint: which offsets are costed never changes a result, encode.hip)
                        const uint32_t w12 = lane < 6 ? __float_as_uint(gl) : (uint32_t)(16 * st.csnroffst() + (st.cbai(0) >> 3));
                        if (lane < 7) reinterpret_cast<uint32_t *>(dp + offsetof(BlkDesc, gain))[lane] = w12;
                    }
                    bd_ok = true;
                }
                rd.seek(sb.bit);
                frame_draws += (uint32_t)sb.draw;
            }

            DK_LAP(4);
            // ---- a failed block leaves zero planes ----
            if (err) { status |= 1u << blk; frame_dead = true; }
            if constexpr (PARSE) {
                if ((err || !bd_ok) && lane == 0) {
                    P.desc[fidx * 6 + blk].flags = BLK_FAILED;
                    // (no descriptor was stored: the word a transcode's encoder reads as its search hint must not be a leftover
                    // of an earlier call - 0 = no hint, see enc_search_kernel)
                    P.desc[fidx * 6 + blk].src_snr = 0u;
                    // (its wavefront of mant_kernel / mantx_kernel reads no mantissas but has staged a share of the frame)
                    P.desc[fidx * 6 + blk].own_bytes = (uint16_t)short_bytes;
                }
            }
            {
                if (err && !PARSE)
                    for (int c = 0; c < n_in; c++)
                        *reinterpret_cast<float4 *>(cblk + (size_t)c * 256 + 4 * lane) = make_float4(0.f, 0.f, 0.f, 0.f);
                if (P.blksw && lane < nfchans)
                    P.blksw[(fidx * 6 + blk) * nfchans + lane] = (uint8_t)(err ? 0 : ((blkswm >> lane) & 1));
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        DK_LAP(5);
        // ac3mi_set_decode_crc: bits 10 / 11 - not for a frame the header test itself refused (crc_kernel repeats that test and
        // does not sum such a frame; the one refusal it cannot see, an output liba52 would not grant, is screened per call by
        // ac3mi_decode_planes - the mask keeps "bit 8 without the verdict's bit 6 = neither bit" whatever the refusal was)
        if (const uint8_t *crcp = crc_verdicts()) {
            const uint32_t cv = crcp[fidx];
            if (!(status & 0x100u) || (cv & 0x40u)) status |= (cv & 3u) << 10;
        }
        if (lane == 0) P.status[fidx] = status | (reuse0 ? 0x200u : 0u);
        if (lane == 0 && P.zs) P.zs[fidx] = (uint8_t)((status & 0x100u) ? 0 : surround_level_is_zero(acm, st.output(), st.slev()));
        if (MODE == 5 && lane == 0) P.frame_draws[fidx] = frame_draws;
        if (MODE == 4) {
            if (lane == 0) P.frame_pos[fidx] = pos_live ? lfsr_pos : 0xffffffffu;
            lfsr_pos = (lfsr_pos + frame_draws) % 65535u;
        }
    }
    if (MODE == 0 && lane == 0) P.lfsr_state[sslot] = (uint16_t)st.lfsr;
    if (MODE == 4 && lane == 0 && pos_live) P.lfsr_state[sslot] = P.lfsr_seq[lfsr_pos];
    DK_END();
}

}  // namespace ac3mi
