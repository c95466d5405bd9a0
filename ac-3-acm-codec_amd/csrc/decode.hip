// decode.hip — AC-3 frame front end on gfx950: BSI + audio-block side information,
// exponent decode, parametric bit allocation, mantissa unpack + dequantisation, dither,
// coupling, rematrixing.  Output: the dequantised, gain-scaled coefficient planes that
// xform.hip turns into PCM.  Replaces a52_frame (L52/parse.c:131-205) and everything in
// a52_block up to the transform stage (L52/parse.c:558-879), a52_bit_allocate
// (L52/bit_allocate.c:124-265) and the bit reader (L52/bitstream.c/.h).
//
// One wavefront (= one 64-thread workgroup) owns one stream and walks its frames in
// order, because the dither LFSR and the exponent / bit-allocation state carry over.
//  * the frame is staged once into (dynamic) LDS as byte-swapped dwords
//  * side information is serial: parsed by all lanes on wave-uniform values through a 64-bit
//    scalar bit window (struct Rd)
//  * exponents: one lane per 7-bit group, DPP prefix sum of the deltas
//  * bit allocation: the whole wavefront per channel (ba_wide_psd + bit_allocate_finish): the band PSDs
//    of two channels per sweep, lowcomp as an automaton evaluated by scans, leaks as prefix minima
//  * mantissas: one sweep, 64 consecutive coefficients of a channel segment per step; two packed
//    DPP scans give grouped-code ranks, bit offsets and dither draw indices (the LFSR is
//    GF(2)-linear, so the k-th draw is a table lookup: lfsr_seq[(lfsr_idx[state] + k) mod 65535]);
//    dequantisation through one table (L1-resident); planes go straight to HBM
//
// Built with -ffp-contract=off: coefficient values are bit-identical to liba52's.
//
// The front-end kernel itself, decode_kernel<MODE, FX, SRC>, is decode_kernel.h; this file instantiates every variant but one
// (decode_src.hip) and holds the rest of the split front end and the launcher.
#include "decode_kernel.h"

namespace ac3mi {

// LFSR state at the start of every frame: one thread per stream walks its frames' draw counts (the generator is
// GF(2)-linear with period 65535: k draws = k positions along the cycle; state 0 is a fixed point).
// frame_pos (split front end): the position along the cycle instead of the state (0xffffffff: state 0), and the stream's
// final state written back here.
__global__ void lfsr_prefix_kernel(const uint32_t *draws, uint16_t *frame_lfsr, uint32_t *frame_pos, uint16_t *lfsr_state, const int32_t *slot,
                                   const uint16_t *seq, const uint16_t *idx, int n_streams, int frames)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_streams) return;
    uint32_t state = lfsr_state[slot ? slot[s] : s];
    uint32_t pos = idx[state];
    for (int f = 0; f < frames; f++) {
        if (frame_pos) frame_pos[(size_t)s * frames + f] = state ? pos : 0xffffffffu;
        else frame_lfsr[(size_t)s * frames + f] = (uint16_t)state;
        const uint32_t k = draws[(size_t)s * frames + f];
        if (state != 0 && k) { pos = (pos + k) % 65535u; state = seq[pos]; }
    }
    if (frame_pos) lfsr_state[slot ? slot[s] : s] = (uint16_t)state;
}

// ---------------------------------------------------------------------------
// mant_kernel: the mantissa half of the split front end.  A workgroup of six wavefronts takes one frame, staged once
// into LDS; wavefront b unpacks, dequantises and stores audio block b from its BlkDesc (mant_block, decode_common.h:
// the code of the one-kernel front ends, rows and coupling coordinates from the workspace).  Nothing carries from one
// block to the next, so the six run concurrently and a wavefront's dependent chain is a sixth of a frame.
struct MantLDS {
    uint4 dsc[M2_NDESC];
    float qtab[760];
    uint8_t ring[6][M2_LDS_WAVE];
    uint8_t cplbnd[6][20];
};

#ifndef MANT_LB
#define MANT_LB 7       // (wavefronts per SIMD the register budget is set for: 8 -> 64 VGPRs but 78 scalar registers with 69 spilled,
#endif                  //  7 -> 71 / 94 / 39, 6 -> 75 / 106 / 28; decode to s16 through this kernel 3.24 / 3.18 / 3.27 ms, round 4)
__global__ __launch_bounds__(384, MANT_LB) void mant_kernel(const MantParams P)
{
    __shared__ MantLDS L;
    extern __shared__ uint32_t frw[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int blk = __builtin_amdgcn_readfirstlane(tid >> 6);
    // consecutive frames on one XCD: its L2 then serves each frame's bytes and rows to the six wavefronts once
    const unsigned fidx = xcd_remap(blockIdx.x, gridDim.x);
    const size_t unit = (size_t)fidx * 6 + blk;
    // the block's descriptor: five 16-byte loads of one address, in flight while the frame is staged
    const uint4 *dq = reinterpret_cast<const uint4 *>(P.desc + unit);
    const BlkWords D{{dq[0], dq[1], dq[2], dq[3], dq[4]}};
    const uint32_t fposv = P.frame_pos[fidx];
    const int nw = (P.frame_bytes + 3) >> 2;
    // the frame's words and the thread's two dequantiser words are all requested before the first is waited for (as
    // mantx_kernel, decode_mx.hip; its earlier row request is not taken over: here it cost 12 bytes of scratch)
    const auto fw = stage_frame_fetch<384>(P.frames + (size_t)fidx * P.frame_stride, P.frame_bytes, tid);
    const float q0 = P.tab->qtab[tid];
    float q1 = 0.f;
    if (tid < 760 - 384) q1 = P.tab->qtab[384 + tid];
    float *cblk = P.coef + unit * P.n_in * 256;
    MantBlk B;
    B.nf = P.nfchans; B.lfeon = P.lfeon; B.acmod = P.acmod; B.in_lfe = P.lfeon ? 1 : 0;
    const bool failed = D.head(B);
    const uint64_t rve = D.rv_exp(), rvb = D.rv_bap();
    const uint8_t *const rowbase = P.rows + (size_t)fidx * 6 * ROWSET;
    const RowFetch fetch{rowbase, rve, rvb, lane};
    {
        stage_frame_store<384>(frw, fw, P.frame_bytes, tid);
        // the slot's bytes behind a frame shorter than frame_bytes are not the frame's.  The parse kernel leaves such a frame's own
        // size in every block's descriptor (0: full size - every frame of a batch of one frame size); each thread clears what it staged
        if (const int own = D.own_bytes()) trim_staged_frame(frw, own, nw, tid, 384);
        if (tid < M2_NDESC) L.dsc[tid] = mant_desc2((uint32_t)tid);
        L.qtab[tid] = q0;
        if (tid < 760 - 384) L.qtab[384 + tid] = q1;
    }
    // the first segment's rows are requested before the workgroup meets at the barrier
    const int slot0 = seg_slot(0, B.nf, B.chincpl, B.chincpl ? __builtin_ctz(B.chincpl) : 99);
    uint2 first = make_uint2(0u, 0u);
    if (!failed) first = fetch(slot0);
    __syncthreads();
    if (failed) {                                               // a failed block leaves zero planes
        for (int c = 0; c < P.n_in; c++)
            *reinterpret_cast<float4 *>(cblk + (size_t)c * 256 + 4 * lane) = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    D.ranges(B);
    B.gainv = D.gainv(lane);
    if (B.chincpl && lane < 18) {                               // sub-band -> band (parse.c:448-456)
        const uint32_t below = D.cplbndstrc() & ((1u << lane) - 1u);
        L.cplbnd[blk][lane] = (uint8_t)(lane - __popc(below));
    }
    const uint32_t fpos = rfl(fposv);
    const bool lfsr_live = fpos != 0xffffffffu;
    const uint32_t i0 = lfsr_live ? (fpos + D.draw_off()) % 65535u : 0u;            // the generator's position before the block's first draw
    const float *cc = P.cplco + unit * 90;
    mant_block2<256, true>(B, fetch, first, [&](int c, int bnd) { return cc[c * 18 + bnd]; }, L.cplbnd[blk], L.dsc, L.ring[blk], frw, (uint32_t)nw + 2u,
                L.qtab, reinterpret_cast<const int16_t *>(P.lfsr_seq) + 1 + i0, lfsr_live, cblk, D.bitpos(), lane);
}

}  // namespace ac3mi

namespace ac3mi {

#ifdef DEC_STAMPS
}  // namespace ac3mi
extern "C" __attribute__((visibility("default"))) int ac3mi_debug_dec_cycles(unsigned long long *out8, int reset)
{
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(ac3mi::g_dec_cycles), sizeof(unsigned long long) * 8) != hipSuccess) return -1;
    if (reset) { unsigned long long z[8] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(ac3mi::g_dec_cycles), z, sizeof z) != hipSuccess) return -1; }
    return 0;
}
namespace ac3mi {
#endif

hipError_t launch_mantx(const DeviceTables &tab, const DecodeLaunch &L, const MantParams &M, const KernelLaunch &k, hipStream_t stream);     // decode_mx.hip
void launch_decode0_src(const DecodeParams &P, unsigned n_streams, size_t fr_bytes, hipStream_t stream);         // decode_src.hip

hipError_t decode_params(const DeviceTables &tab, const DecodeLaunch &L, DecodeParams &P)
{
    if (L.frame_bytes > STAGE_MAX_BYTES) return hipErrorInvalidValue;      // (stage_frame's fixed words per thread; the C entry points refuse it first)
    const bool split = L.choice.split;
    P.desc = split ? (BlkDesc *)L.ws_desc : nullptr;
    P.rows = split ? L.ws_rows : nullptr;
    P.cplco = split ? L.ws_cplco : nullptr;
    P.frame_pos = split ? L.ws_fpos : nullptr;
    P.frames = L.frames;
    P.coef = L.coef;
    P.blksw = L.blksw;
    P.zs = L.zs;
    P.status = L.status;
    P.lfsr_state = L.lfsr;
    P.slot = L.slot;
    P.tap_exp = L.tap_exp;
    P.tap_bap = L.tap_bap;
    P.lfsr_seq = tab.lfsr_seq;
    P.lfsr_idx = tab.lfsr_idx;
    P.tab = tab.dec;
    P.n_streams = L.n_streams;
    P.frames_per_stream = L.frames_per_stream;
    P.frame_stride = L.frame_stride;
    P.frame_bytes = L.frame_bytes;
    P.req_flags = L.req_flags;
    P.level = L.level;
    P.dynrng_on = L.dynrng_on;
    P.acmod = L.acmod;
    P.lfeon = L.lfeon;
    P.nfchans = sync_nfchans(L.acmod & 7);
    P.n_in = P.nfchans + (L.lfeon ? 1 : 0);
    P.frame_draws = L.frame_draws;
    P.frame_lfsr = L.frame_lfsr;
    P.dyn_out = L.dyn_out;
    P.dyn_in = L.dyn_in;
    P.crc = L.crc;
    if (L.src_dyn) {                    // the raw words take the tap's slot: never with gains applied, or with the tap
        if (L.dynrng_on || L.dyn_out || L.dyn_in) return hipErrorInvalidValue;
        P.src_dyn = L.src_dyn;
    }
    return hipSuccess;
}

// decode_kernel under a word of DECODE_VARIANTS (null: decode_src.hip's, launched there)
template <uint32_t V> constexpr auto decode_variant()
{
    using Fn = void (*)(DecodeParams);
    if constexpr (V == V_SRC) return (Fn) nullptr;
    else return (Fn)decode_kernel<(int)(V & V_NUM), (V & V_FX) != 0, (V & V_SRC) != 0>;
}
template <uint32_t V> struct DecodeVariant { static constexpr auto fn = decode_variant<V>(); };

// the kernels of L.choice (launch_rule.h: dec_choice) in order
hipError_t launch_decode(const DeviceTables &tab, const DecodeLaunch &L, hipStream_t stream)
{
    DecodeParams P;
    const hipError_t ep = decode_params(tab, L, P);
    if (ep != hipSuccess) return ep;
    if (L.n_streams <= 0 || L.frames_per_stream <= 0) return hipSuccess;
    const DecChoice &c = L.choice;
    if (c.err || c.wg) return hipErrorInvalidValue;
    static const int lds_pad = getenv("AC3MI_DEC_LDS_PAD") ? atoi(getenv("AC3MI_DEC_LDS_PAD")) : 0;      // profiling aid: occupancy sweeps
    static const int mant_pad = getenv("AC3MI_MANT_LDS_PAD") ? atoi(getenv("AC3MI_MANT_LDS_PAD")) : 0;      // profiling aid: occupancy proxy of a fused mantissa + transform workgroup
    const size_t fr_bytes = staged_frame_lds(L.frame_bytes);
    for (int i = 0; i < c.n; i++) {
        const KernelLaunch &k = c.launch[i];
        const dim3 grid(grid_size(k, L.n_streams, L.frames_per_stream, 1)), block(k.block);
        if (k.family == K_DECODE && k.variant == V_SRC) {
            log_launch(L.log, k);
            launch_decode0_src(P, grid.x, fr_bytes + lds_pad, stream);
        }
        else if (k.family == K_DECODE) {
            const auto fn = variant_fn<DECODE_VARIANTS, DecodeVariant>(k.variant);
            if (!fn) return hipErrorInvalidValue;
            log_launch(L.log, k);
            hipLaunchKernelGGL(fn, grid, block, fr_bytes + lds_pad, stream, P);
        } else if (k.family == K_LFSR_PREFIX) {
            log_launch(L.log, k);
            hipLaunchKernelGGL(lfsr_prefix_kernel, grid, block, 0, stream, (const uint32_t *)L.frame_draws, (uint16_t *)nullptr, L.ws_fpos,
                               L.lfsr, L.slot, tab.lfsr_seq, tab.lfsr_idx, L.n_streams, L.frames_per_stream);
        } else if (k.family == K_MANT || k.family == K_MANTX) {
            MantParams M;
            M.frames = L.frames;
            M.desc = (const BlkDesc *)L.ws_desc;
            M.rows = L.ws_rows;
            M.cplco = L.ws_cplco;
            M.frame_pos = L.ws_fpos;
            M.coef = L.coef;
            M.lfsr_seq = tab.lfsr_seq;
            M.tab = tab.dec;
            M.n_frames = grid.x;
            M.frame_stride = L.frame_stride;
            M.frame_bytes = L.frame_bytes;
            M.acmod = L.acmod;
            M.lfeon = L.lfeon;
            M.n_in = P.n_in;
            M.nfchans = P.nfchans;
            if (k.family == K_MANTX) return launch_mantx(tab, L, M, k, stream);     // the transform in the same kernel
            log_launch(L.log, k);
            hipLaunchKernelGGL(mant_kernel, grid, block, fr_bytes + mant_pad, stream, M);
        } else return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace ac3mi
