// launch_rule.h — which kernel variants a batch call launches, stated once: the instantiations that exist (one list per
// kernel family), the decoder's front end (dec_choice) and the encoder's chain (enc_choice).  Every choice here is between
// kernels that return the same bytes, so no byte test can tell a wrong one; tests/launch_rule_c holds the rule to a table
// recorded from the launchers it replaced.  The launchers (decode.hip, decode_mx.hip, decode_wg.hip, encode.hip) ask the rule,
// fill their parameter structs and launch what variant_fn finds under the variant word; capi.hip sizes the workspaces from
// the same answer.
// Plain C++17: compiles without HIP (the sanitiser program of tests/launch_rule_c includes it).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <array>
#include <utility>
#include "sync_rule.h"

namespace ac3mi {

// A variant word: the template arguments of one instantiation, one bit per bool parameter under the parameter's name;
// bits 0-2 are the family's int parameter (decode_kernel's MODE, decode_wg_kernel's OUT, enc_search_kernel's PART).
enum : uint32_t {
    V_NUM = 7u, V_FX = 1u << 3, V_SRC = 1u << 4, V_S16 = 1u << 5, V_BSW = 1u << 6, V_REMAT = 1u << 7, V_BW = 1u << 8, V_XS = 1u << 9,
    V_LFEROW = 1u << 10, V_R3 = 1u << 11, V_CPL = 1u << 12, V_DRC = 1u << 13, V_DW = 1u << 14, V_MD = 1u << 15, V_DUAL = 1u << 16,
};

// The instantiations that exist.  A launcher's table is built over its list (variant_fn below), so a variant is named here
// and nowhere else.
// decode_kernel<MODE, FX, SRC> (V_SRC alone - MODE 0 with SRC - is decode_src.hip's: a translation unit of its own, see there)
inline constexpr uint32_t DECODE_VARIANTS[] = {0, V_SRC, 4, 4 | V_FX, 4 | V_SRC, 5, 5 | V_SRC};
// decode_wg_kernel<OUT, SRC>: OUT 0 planes, 1 float PCM, 2 s16 PCM
inline constexpr uint32_t DECODE_WG_VARIANTS[] = {0, 1, 2, 2 | V_SRC};
// mantx_kernel<S16, FX>; mant_kernel and lfsr_prefix_kernel are no templates: one word, 0
inline constexpr uint32_t MANTX_VARIANTS[] = {0, V_S16, V_S16 | V_FX};
inline constexpr uint32_t PLAIN_VARIANT[] = {0};
// enc_mdct_kernel<BSW, REMAT, BW, XS, LFEROW, FX>
inline constexpr uint32_t ENC_MDCT_VARIANTS[] = {
    0, V_FX, V_BSW, V_REMAT, V_BSW | V_REMAT, V_REMAT | V_BW, V_BSW | V_REMAT | V_BW,
    V_XS, V_XS | V_BSW, V_XS | V_REMAT, V_XS | V_BSW | V_REMAT, V_XS | V_REMAT | V_BW, V_XS | V_BSW | V_REMAT | V_BW,
    V_LFEROW, V_LFEROW | V_XS};
// enc_cpl_kernel<BW, XS, R3>
inline constexpr uint32_t ENC_CPL_VARIANTS[] = {0, V_BW, V_XS, V_BW | V_XS, V_R3, V_R3 | V_BW, V_R3 | V_XS, V_R3 | V_BW | V_XS};
// enc_search_kernel<PART, CPL, BW, DRC, FX, DW>: six of each words rule (none, DRC, DRC and DW), and the fixed-shape search
#define AC3MI_SEARCH6(W) 1 | (W), 1 | V_CPL | (W), 1 | V_CPL | V_BW | (W), 3 | (W), 3 | V_CPL | (W), 3 | V_CPL | V_BW | (W)
inline constexpr uint32_t ENC_SEARCH_VARIANTS[] = {AC3MI_SEARCH6(0u), AC3MI_SEARCH6(V_DRC), AC3MI_SEARCH6(V_DRC | V_DW), 1 | V_FX};
#undef AC3MI_SEARCH6
// enc_packf_kernel<FIXED51 (V_FX), CPL, BW, MD, DUAL, DW>
#define AC3MI_PACKF6(W) (W), V_DUAL | (W), V_FX | (W), V_FX | V_BW | (W), V_CPL | (W), V_CPL | V_BW | (W)
inline constexpr uint32_t ENC_PACKF_VARIANTS[] = {AC3MI_PACKF6(0u), AC3MI_PACKF6(V_MD), AC3MI_PACKF6(V_MD | V_DW)};
#undef AC3MI_PACKF6
// enc_packb_kernel<MD, DW>
inline constexpr uint32_t ENC_PACKB_VARIANTS[] = {0, V_MD, V_MD | V_DW};

// The kernel under a variant word: K<V>::fn is the family's instantiation for word V; the table holds K<LIST[i]>::fn for the
// listed words and nothing else is instantiated.  Null: the word is not in the list (the launcher returns an error; the
// test shows the rule returns listed words only).
template <const auto &LIST, template <uint32_t> class K, size_t... I>
constexpr auto variant_table(std::index_sequence<I...>) { return std::array<decltype(K<LIST[0]>::fn), sizeof...(I)>{{K<LIST[I]>::fn...}}; }
template <const auto &LIST, template <uint32_t> class K>
inline decltype(K<LIST[0]>::fn) variant_fn(uint32_t v)
{
    static constexpr auto T = variant_table<LIST, K>(std::make_index_sequence<std::size(LIST)>{});
    for (size_t i = 0; i < std::size(LIST); i++)
        if (LIST[i] == v) return T[i];
    return nullptr;
}

enum KernelFamily : uint8_t {
    K_NONE, K_DECODE, K_DECODE_WG, K_LFSR_PREFIX, K_MANT, K_MANTX, K_ENC_MDCT, K_ENC_CPL, K_ENC_SEARCH, K_ENC_PACKF, K_ENC_PACKB
};
// what a launch has one workgroup for: a stream, a frame, a channel of a frame, 64 streams (lfsr_prefix_kernel), or a
// stream up to as many workgroups as the chip holds at once (decode_wg_kernel's persistent grid)
enum GridUnit : uint8_t { G_STREAM, G_FRAME, G_CHANNEL, G_64_STREAMS, G_RESIDENT };
struct KernelLaunch {
    uint8_t family = K_NONE, grid = G_STREAM;
    uint16_t block = 0;
    uint32_t variant = 0;
};
inline constexpr KernelLaunch kernel_launch(KernelFamily f, uint32_t v, GridUnit g, int block) { return KernelLaunch{f, g, (uint16_t)block, v}; }
inline constexpr unsigned grid_size(const KernelLaunch &l, int n_streams, int frames_per_stream, int nch)
{
    const unsigned nfr = (unsigned)n_streams * (unsigned)frames_per_stream;
    return l.grid == G_FRAME ? nfr : l.grid == G_CHANNEL ? nfr * (unsigned)nch : l.grid == G_64_STREAMS ? ((unsigned)n_streams + 63u) / 64u : (unsigned)n_streams;
}

// The launch log (ac3mi_debug_launch_log, a test aid): `words` is host memory of `capacity` words; words[0] counts the launches
// since the tap was set, those that no longer fit included, words[1..] holds family << 24 | variant word of each in launch
// order.  The launchers call log_launch where they resolve variant_fn (and at the two plain kernels' launches), on the host
// thread that makes the batch call: nothing on the device, and a null log costs one test.
struct LaunchLog {
    uint32_t *words = nullptr;
    int capacity = 0;
};
inline constexpr uint32_t launch_word(uint8_t family, uint32_t variant) { return (uint32_t)family << 24 | variant; }
inline void log_launch(const LaunchLog *log, const KernelLaunch &k)
{
    if (!log || !log->words) return;
    const uint32_t n = ++log->words[0];
    if (n < (uint32_t)log->capacity) log->words[n] = launch_word(k.family, k.variant);
}

// dynamic LDS of a kernel that stages a frame (stage_frame, decode_common.h): its dwords and six of slack for the bit window
inline constexpr size_t staged_frame_lds(int frame_bytes) { return (size_t)(((frame_bytes + 3) >> 2) + 6) * 4; }

// The shape large batches run at - 5.1: acmod 7 with the LFE, six planes in and out, five full-bandwidth channels.  The one
// predicate behind every kernel variant that has it compiled in (ac3mi_set_fixed_shape): dec_choice and enc_choice add their
// own conditions - one frame per stream, the stage's tools and taps off - and anything else takes the generic kernels.
inline constexpr bool fixed51_shape(int acmod, int lfeon, int n_in, int n_out, int nfbw)
{
    return acmod == 7 && lfeon != 0 && n_in == 6 && n_out == 6 && nfbw == 5;
}

// ---------------------------------------------------------------------------
// The decoder front end of a call.
struct DecChoice {
    bool identity = false;      // every coded plane is an output plane
    bool mixstate = false;      // liba52's overlap bookkeeping around frames with surround level 0 (ac3mi_set_mix_state)
    bool wg = false, fused = false;     // decode_wg.hip; with the transform fused in (no workspace at all)
    bool split = false, mantx = false;  // the split front end; its mantissa kernel with the transform fused in
    bool fp = false;            // frame-parallel
    bool err = false;           // the launcher refuses the call (hipErrorInvalidValue) before its first launch
    int n = 0;
    KernelLaunch launch[3];     // the front end's kernels in order (the transform kernel, where it follows, is the caller's)
};

// The split front end's mantissa kernel with the transform fused in (decode_mx.hip: no coefficient planes in HBM)?  Needs
// one-frame streams (a block's overlap tail goes to the next block inside the frame's workgroup) and every coded plane an output
// plane.  Mode 6: wherever that holds; auto: for s16 output only - measured per 65 536 5.1 frames (profiles/r04_kernel_stats.csv,
// profiles/EXPERIMENTS.md): to s16 2.12 - 2.17 ms fused against 1.31 + 0.77 = 2.08 - 2.15 ms in two kernels (a wash in time,
// 36.9 KB per frame less HBM traffic and workspace), to float 2.45 against 1.31 + 0.97 = 2.28 ms (the two kernels stay);
// modes 4 / 5 always keep the two kernels (the bit-identity reference, A/B runs).
inline constexpr bool dec_mantx(int mode, int frames_per_stream, bool identity, bool s16)
{
    return ((mode == 0 && s16) || mode == 6) && frames_per_stream == 1 && identity;
}

// mode: ac3mi_set_decode_mode.  taps: the call writes stage taps; wg_planes: the one-workgroup-per-stream kernel may also
// write coefficient planes for the transform kernel (decode) - else it is taken only with the transform fused in (transcode);
// identity: the mix plan routes every coded plane to its own output plane; mix_state: ac3mi_set_mix_state is on and the plan
// has surround planes it bears on; src: the front end leaves the raw dynamic-range words (DecodeLaunch::src_dyn).
inline DecChoice dec_choice(int mode, int n_streams, int frames_per_stream, bool s16, bool taps, bool wg_planes, bool identity,
                            bool mix_state, bool fixed_shape, int acmod, int lfeon, bool src)
{
    DecChoice c;
    c.identity = identity;
    c.mixstate = mix_state && !identity;
    // One workgroup per stream (decode_wg.hip)?  Its eight wavefronts cut the latency of a frame to a third and nothing but the
    // frame and the PCM touches HBM, but a workgroup's wavefronts wait for each other at the block's barriers, so the chip holds
    // fewer busy wavefronts than the other front ends.  Measured on one-frame streams to s16 (round 3, profiles/decode_ab.py;
    // fused / split front end + transform / one-kernel front end + transform): 64 streams 0.084 / 0.118 / 0.167 ms, 256: 0.086 /
    // 0.121 / 0.165, 1 024: 0.188 / 0.150 / 0.184, 2 048: 0.362 / 0.186 / 0.206, 4 096: 0.70 / 0.28 / 0.28, 65 536: 10.7 / 3.5 / 4.2.
    // auto: batches of up to 512 streams of at most four frames (round 2: 1 024, against the one-kernel front end); mode 3 forces it.
    c.wg = (mode ? mode == 3 : n_streams <= 512 && frames_per_stream <= 4) && (wg_planes || identity);
    c.fused = c.wg && identity && !taps;
    // Split front end (parse kernel, then one wavefront per audio block: decode_kernel MODE 4 / 5 + mant_kernel)?  auto: yes;
    // mode 1 forces the one-kernel front end (one wavefront per stream), 4 / 5 the split one per stream / per frame.
    c.split = !c.wg && (mode == 0 || mode >= 4);
    c.mantx = c.split && !taps && dec_mantx(mode, frames_per_stream, identity, s16);
    // Frame-parallel front end for few long streams?  auto: more than one frame per stream and too few streams to fill the
    // chip with one wavefront each (256 CUs x 20 wavefronts); mode 5 forces it, also for one-frame streams (A/B runs).
    c.fp = !c.wg && (mode ? mode == 5 : frames_per_stream >= 2 && n_streams < 5120);
    if (n_streams <= 0 || frames_per_stream <= 0) return c;
    auto add = [&c](KernelFamily f, uint32_t v, GridUnit g, int block) { c.launch[c.n++] = kernel_launch(f, v, g, block); };
    const uint32_t vsrc = src ? V_SRC : 0u;
    if (c.wg) {
        // the raw words are a transcode's: s16 PCM from the fused kernel
        if (src && !(c.fused && s16)) c.err = true;
        else add(K_DECODE_WG, (c.fused ? (s16 ? 2u : 1u) : 0u) | vsrc, G_RESIDENT, 512);
        return c;
    }
    if (!c.split) {
        // (rounds 1-2 also had a one-kernel front end per FRAME for few long streams - counting pass, generator prefix, full pass;
        // the split front end's per-frame parse kernel replaced it in round 3 and it was retired in round 4)
        if (c.fp) c.err = true;
        else add(K_DECODE, 0u | vsrc, G_STREAM, 64);
        return c;
    }
    // The fixed-shape rule (ac3mi_set_fixed_shape): one-frame 5.1 streams whose six planes are the output's (the fused
    // kernel's calls), no stage taps - parse and mantissa kernel with that shape compiled in.  Same results either way
    const int nf = sync_nfchans(acmod), n_in = nf + (lfeon ? 1 : 0);
    const bool fx = !src && fixed_shape && c.mantx && fixed51_shape(acmod, lfeon, n_in, n_in, nf);
    // parse (per stream, or per frame + the generator's prefix), then one wavefront per audio block
    if (!c.fp) add(K_DECODE, 4u | (fx ? V_FX : vsrc), G_STREAM, 64);
    else {
        add(K_DECODE, 5u | vsrc, G_FRAME, 64);
        add(K_LFSR_PREFIX, 0, G_64_STREAMS, 64);
    }
    // one-frame streams, no downmix: the transform in the same kernel
    if (c.mantx) add(K_MANTX, s16 ? V_S16 | (fx ? V_FX : 0u) : 0u, G_FRAME, 384);
    else add(K_MANT, 0, G_FRAME, 384);
    return c;
}

// ---------------------------------------------------------------------------
// The encoder's chain of a call.
enum EncStage { ES_PRE, ES_MDCT, ES_LFEROW, ES_CPL, ES_TABULATE, ES_SEARCH, ES_PACK, ES_COUNT };
struct EncChoice {
    bool err = false;           // launch_encode refuses the call (hipErrorInvalidValue) before its first launch
    int nbc = 0, cpl_endf = 0;  // coefficients per full-bandwidth channel; where a coupled frame ends at this bandwidth
    bool bw = false;            // the variants whose coupling end or 5.1 band edge is a run-time value
    bool cpl = false;           // the call couples
    bool drc = false, dw = false, md = false;   // DRC profile on; words from arrays; the packers write metadata
    bool remat = false;         // rematrixing bears on the layout (2/0, with or without the LFE)
    bool packb = false;         // the block packer (else one wavefront per frame)
    bool memo = false;          // the tabulating search runs first
    bool history = false;       // enc_history_kernel follows (streams of more than one frame)
    KernelLaunch stage[ES_COUNT];       // in launch order; family K_NONE: the stage does not run
};

// the encoder's BSI fields (ac3mi_set_encode_metadata) in one word: dialnorm bits 0-4, bsmod 5-7, cmixlev 8-9, surmixlev
// 10-11, dsurmod 12-13, copyrightb 14, origbs 15
constexpr uint32_t bsi_word(int dialnorm, int bsmod, int cmixlev, int surmixlev, int dsurmod, int copyrightb, int origbs)
{
    return (uint32_t)dialnorm | (uint32_t)bsmod << 5 | (uint32_t)cmixlev << 8 | (uint32_t)surmixlev << 10 |
           (uint32_t)dsurmod << 12 | (uint32_t)copyrightb << 14 | (uint32_t)origbs << 15;
}
constexpr uint32_t BSI_DEFAULT = bsi_word(31, 0, 1, 1, 0, 0, 1);      // the reference's fixed BSI: any other word, the MD packers

// the packers' member lists (enc_mant.h) hold the grouped mantissas of at most 5 x 223 + 7 coefficients a block
constexpr int ENC_MAX_COEFS = 5 * 223 + 7;

// in: the call as launch_encode gets it (EncodeLaunch, ac3mi_internal.h), read by member name - cfg.acmod / lfe / nch / nfbw,
// n_streams, frames_per_stream, pack_mode, chbwcod, bw, cpl_begf, drc_profile, bsi, exp_strategy, fixed_shape, mdct_full_rows,
// and of ws_bsw, ws_remat, dyn_codes, compr_words, bsi_words, ws_expo, tap_strat, tap_snr and ws_memo whether they are set
template <class Call> inline EncChoice enc_choice(const Call &in)
{
    const auto &cfg = in.cfg;
    EncChoice c;
    if (in.n_streams <= 0 || in.frames_per_stream <= 0) return c;
    // the call's bandwidth (ac3mi_set_encode_bandwidth): nbc coefficients per full-bandwidth channel, a coupled frame ends at
    // cplendf.  bw on, or any chbwcod below 50: the runtime-bandwidth variants run (mode 0 launches exactly the kernels it always did)
    if (in.chbwcod < 0 || in.chbwcod > 50) { c.err = true; return c; }
    c.nbc = 73 + 3 * in.chbwcod;
    c.cpl_endf = in.chbwcod >> 2 < 12 ? in.chbwcod >> 2 : 12;
    c.bw = in.bw || in.chbwcod != 50;
    if (cfg.nfbw * c.nbc + 7 > ENC_MAX_COEFS) { c.err = true; return c; }
    // metadata and dynamic range control: the DRC kernels write the frames' codes first; with DRC on the search costs the words
    // (DRC variants), with either on, or a word per frame (bsi_words), the packers write them (MD variants).  Words from the
    // caller's or the source's arrays (dyn_codes / compr_words): the DW variants of the search and the packers, which cost and
    // write them.  All off: exactly the kernels of before
    c.dw = in.dyn_codes || in.compr_words;
    if (in.dyn_codes && in.drc_profile) { c.err = true; return c; }        // (the C API refuses the pair)
    c.drc = in.drc_profile != 0;
    c.md = c.dw || c.drc || in.bsi != BSI_DEFAULT || in.bsi_words;
    c.remat = cfg.acmod == 2 && in.ws_remat;     // (rematrixing is a 2/0 tool, with or without the LFE: other layouts ignore it)
    // The fixed-shape rule (ac3mi_set_fixed_shape): a 5.1 call takes the kernels that have that shape compiled in
    // (the FX / FIXED51 instantiations) - the front kernel and the search when, besides, the streams are one frame long, the
    // bandwidth is the full one and no tool of theirs is on (fx_plain; each adds "no stage tap of mine" below).  Same bytes either way
    const bool fixed51 = in.fixed_shape && fixed51_shape(cfg.acmod, cfg.lfe, cfg.nch, cfg.nch, cfg.nfbw);
    const bool fx_plain = fixed51 && in.frames_per_stream == 1 && !c.bw && !in.ws_bsw && !in.ws_remat && in.cpl_begf < 0 && !c.drc &&
                          !c.dw && !in.exp_strategy;
    // (begf > cplendf + 2: no coupling band - no frame couples, the bytes are coupling off's; dual mono's two programmes are
    // never coupled)
    c.cpl = in.cpl_begf >= 0 && cfg.nfbw >= 2 && cfg.acmod != 0 && in.cpl_begf <= c.cpl_endf + 2;
    const uint32_t vbsw = in.ws_bsw ? V_BSW : 0u, vxs = in.exp_strategy ? V_XS : 0u, vbw = c.bw ? V_BW : 0u;
    // coupling with rematrixing: the rows without rematrixing first (before the history is rewritten), for enc_cpl_kernel.
    // (The pre-pass keeps mode 0's strategy rule: of its exponent stage only the rows and exp_samples are read)
    if (c.cpl && c.remat) c.stage[ES_PRE] = kernel_launch(K_ENC_MDCT, vbsw, G_CHANNEL, 64);
    // the front kernel: a workgroup per channel, or with rematrixing two wavefronts per frame
    uint32_t v = vbsw | vxs | (c.remat ? V_REMAT | vbw : 0u);
    if (!v && fx_plain && !in.mdct_full_rows && !in.ws_expo) v = V_FX;
    c.stage[ES_MDCT] = c.remat ? kernel_launch(K_ENC_MDCT, v, G_FRAME, 128) : kernel_launch(K_ENC_MDCT, v, G_CHANNEL, 64);
    // 2/0+LFE with rematrixing: the REMAT workgroups code channels 0 and 1, a launch of the plain kernel the LFE row beside them
    if (c.remat && cfg.lfe) c.stage[ES_LFEROW] = kernel_launch(K_ENC_MDCT, V_LFEROW | vxs, G_FRAME, 64);
    // channel coupling: layouts with two or more full-bandwidth channels (R3: 2/0+LFE with rematrixing, three rows a block in
    // the rematrixing arrays)
    if (c.cpl) c.stage[ES_CPL] = kernel_launch(K_ENC_CPL, vbw | vxs | (c.remat && cfg.lfe ? V_R3 : 0u), G_FRAME, 64);    // The SNR-offset searches run one wavefront per stream (PART 1; for few long streams behind PART 3's frame-parallel
    // tabulation, worth its cost only when the per-stream replay is the long pole), then every frame is packed.
    // (the uncoupled search and enc_packb_kernel take nbc / chbwcod at run time in every mode)
    c.memo = in.frames_per_stream > 1 && in.n_streams < 2048 && in.ws_memo;
    const uint32_t vcpl = c.cpl ? V_CPL | vbw : 0u;
    const uint32_t vwords = c.dw ? V_DRC | V_DW : c.drc ? V_DRC : 0u;
    if (c.memo) c.stage[ES_TABULATE] = kernel_launch(K_ENC_SEARCH, 3u | vcpl | vwords, G_FRAME, 64);
    const bool fx_search = !c.cpl && !vwords && fx_plain && !c.memo && !in.tap_strat && !in.tap_snr;
    c.stage[ES_SEARCH] = kernel_launch(K_ENC_SEARCH, fx_search ? 1u | V_FX : 1u | vcpl | vwords, G_STREAM, 64);
    // The packers: a workgroup of six wavefronts, one per audio block (enc_packb_kernel), or one wavefront per frame
    // (enc_packf_kernel).  Measured per call on one-frame streams, cold (profiles/encode_cold.py, end of round 3): 64 frames
    // 0.107 against 0.162 ms with one wavefront per frame, 256: 0.111 / 0.168, 512: 0.134 / 0.179, 1 024: 0.191 / 0.192,
    // 2 048: 0.291 / 0.262, 4 096: 0.497 / 0.394, 8 192: 0.917 / 0.700 - a frame's chain is a sixth as long, but a workgroup's
    // wavefronts wait for each other five times per frame, so the chip holds fewer busy wavefronts: the block packer takes
    // batches of up to 1 024 frames (the byte-stream layer's chunks), one wavefront per frame the rest.
    // pack_mode (ac3mi_set_encode_mode): 0 = that rule, 1 = never, 2 = always the block packer.  Coupled frames are packed by
    // enc_packf_kernel only.  (Rounds 1-3 also had a one-kernel packer per stream; it held neither half's registers comfortably.)
    const unsigned nfr = (unsigned)in.n_streams * (unsigned)in.frames_per_stream;
    c.packb = !c.cpl && (in.pack_mode == 2 || (in.pack_mode == 0 && nfr <= 1024));
    const uint32_t vmd = c.dw ? V_MD | V_DW : c.md ? V_MD : 0u;
    if (c.packb) c.stage[ES_PACK] = kernel_launch(K_ENC_PACKB, vmd, G_FRAME, 384);
    else {
        const uint32_t shape = c.cpl ? vcpl : fixed51 && c.bw ? V_FX | V_BW : fixed51 && c.nbc == 223 ? V_FX : cfg.acmod == 0 ? V_DUAL : 0u;
        c.stage[ES_PACK] = kernel_launch(K_ENC_PACKF, shape | vmd, G_FRAME, 64);
    }
    // the new history: the front kernel stores it for one-frame streams, else a kernel of its own after the packer
    c.history = in.frames_per_stream != 1;
    return c;
}

}  // namespace ac3mi
