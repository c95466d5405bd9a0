// grid.h — the rows on which the launch rule (csrc/launch_rule.h) is held to the launchers it replaced, and the canonical
// line of a row.  Plain C++ and nothing of the engine: main.cpp walks these rows with the rule; the table beside it
// (parent_table.txt) was made by walking the same rows with the former launch_decode / launch_mantx / launch_decode_wg /
// launch_encode and capi.hip's former front_end(), compiled for the host with hipLaunchKernelGGL turned into a recorder of
// (kernel symbol, grid, block) and hipGetLastError into hipSuccess.
//
// A grid is a mixed-radix index space: digit k of index i picks the value of dimension k.  The full grids (every value of every
// dimension crossed: 264 241 152 encoder rows, 294 912 decoder rows) were compared once; the committed test walks every
// ENC_STRIDE-th / DEC_STRIDE-th index (strides coprime to every radix, so each value of each dimension and each pair keeps
// turning up) and a block of rows with every encoder tool off.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

namespace grid {

struct Launched {
    std::string kernel;         // as the symbol demangles, without namespace and argument list: enc_cpl_kernel<true, false, false>
    unsigned grid, block;
};

// ---- encoder -------------------------------------------------------------------------------------------------------
struct EncRow {
    int acmod, lfe, frames, streams, pack_mode, chbwcod, bw, bsw, remat, begf, drc, dyn, compr, bsi_words, bsi_default, xs, fixed,
        full_rows, expo, tap_strat, tap_snr;
    int nfbw() const { static const int n[8] = {2, 1, 2, 3, 3, 4, 4, 5}; return n[acmod]; }
    int nch() const { return nfbw() + lfe; }
};
static const int ENC_FRAMES[3] = {1, 2, 5};
// per frames-per-stream value: one stream, both sides of 1 024 frames, of 2 048 and of 5 120 streams
static const int ENC_STREAMS[3][7] = {{1, 1024, 1025, 2047, 2048, 5119, 5120}, {1, 512, 513, 2047, 2048, 5119, 5120}, {1, 204, 205, 2047, 2048, 5119, 5120}};
static const int ENC_CHBW[4] = {50, 49, 20, 0};
static const int ENC_BEGF[4] = {-1, 0, 7, 12};
static const int ENC_RADIX[21] = {8, 2, 3, 7, 3, 4, 2, 2, 2, 4, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2};
inline uint64_t enc_rows()
{
    uint64_t n = 1;
    for (int r : ENC_RADIX) n *= (uint64_t)r;
    return n;
}
inline EncRow enc_row(uint64_t i)
{
    int d[21];
    for (int k = 0; k < 21; k++) { d[k] = (int)(i % ENC_RADIX[k]); i /= ENC_RADIX[k]; }
    EncRow r;
    r.acmod = d[0]; r.lfe = d[1]; r.frames = ENC_FRAMES[d[2]]; r.streams = ENC_STREAMS[d[2]][d[3]]; r.pack_mode = d[4];
    r.chbwcod = ENC_CHBW[d[5]]; r.bw = d[6]; r.bsw = d[7]; r.remat = d[8]; r.begf = ENC_BEGF[d[9]]; r.drc = d[10] ? 3 : 0;
    r.dyn = d[11]; r.compr = d[12]; r.bsi_words = d[13]; r.bsi_default = !d[14]; r.xs = d[15]; r.fixed = !d[16];
    r.full_rows = d[17]; r.expo = d[18]; r.tap_strat = d[19]; r.tap_snr = d[20];
    return r;
}
constexpr uint64_t ENC_STRIDE = 2749;       // prime
// every index of the first five dimensions (layout, frames, streams, pack mode) with all the later digits 0 - no tool, no tap,
// the full bandwidth, the fixed shape allowed: the rows the fixed-shape front kernel and search need - and the same with the
// fixed shape refused
template <class F> void enc_reduced(F f)
{
    const uint64_t n = enc_rows();
    for (uint64_t i = 0; i < n; i += ENC_STRIDE) f(enc_row(i));
    for (uint64_t i = 0; i < 8 * 2 * 3 * 7 * 3; i++) {
        EncRow r = enc_row(i);
        f(r);
        r.fixed = 0;
        f(r);
    }
    // rows the rule refuses: chbwcod out of range on either side
    for (int cb : {-1, 51}) {
        EncRow r = enc_row(0);
        r.chbwcod = cb;
        f(r);
    }
}
inline std::string enc_line(const EncRow &r, bool err, const std::vector<Launched> &l, bool history)
{
    char b[160];
    snprintf(b, sizeof b, "E a%d%d F%d S%d P%d C%d%d t%d%d g%d d%d%d%d%d%d x%d f%d T%d%d%d%d |", r.acmod, r.lfe, r.frames, r.streams, r.pack_mode,
             r.chbwcod, r.bw, r.bsw, r.remat, r.begf, r.drc, r.dyn, r.compr, r.bsi_words, r.bsi_default, r.xs, r.fixed, r.full_rows, r.expo,
             r.tap_strat, r.tap_snr);
    std::string s = b;
    if (err) return s + " refused";
    for (const Launched &k : l) s += " " + k.kernel + " " + std::to_string(k.grid) + "x" + std::to_string(k.block) + ";";
    return s + (history ? " history" : "");
}

// ---- decoder -------------------------------------------------------------------------------------------------------
struct DecRow {
    int mode, streams, frames, s16, taps, transcode, identity, mix_state, fixed, acmod, lfe, src;
};
static const int DEC_MODES[6] = {0, 1, 3, 4, 5, 6};
static const int DEC_STREAMS[6] = {1, 512, 513, 5119, 5120, 65536};
static const int DEC_FRAMES[4] = {1, 2, 4, 5};
static const int DEC_RADIX[12] = {6, 6, 4, 2, 2, 2, 2, 2, 2, 8, 2, 2};
inline uint64_t dec_rows()
{
    uint64_t n = 1;
    for (int r : DEC_RADIX) n *= (uint64_t)r;
    return n;
}
// (a transcode is to s16 and has no taps: its rows take those two digits as they come and overrule them)
inline DecRow dec_row(uint64_t i)
{
    int d[12];
    for (int k = 0; k < 12; k++) { d[k] = (int)(i % DEC_RADIX[k]); i /= DEC_RADIX[k]; }
    DecRow r;
    r.mode = DEC_MODES[d[0]]; r.streams = DEC_STREAMS[d[1]]; r.frames = DEC_FRAMES[d[2]]; r.s16 = d[3]; r.taps = d[4]; r.transcode = d[5];
    r.identity = d[6]; r.mix_state = d[7]; r.fixed = !d[8]; r.acmod = d[9]; r.lfe = d[10]; r.src = d[11];
    if (r.transcode) { r.s16 = 1; r.taps = 0; }
    return r;
}
constexpr uint64_t DEC_STRIDE = 7;
template <class F> void dec_reduced(F f)
{
    const uint64_t n = dec_rows();
    for (uint64_t i = 0; i < n; i += DEC_STRIDE) f(dec_row(i));
}
// flags: the front end's seven answers (identity, mixstate, wg, fused, split, mantx, fp), which size the call's workspaces
inline std::string dec_line(const DecRow &r, const char *flags, bool err, const std::vector<Launched> &l)
{
    char b[160];
    snprintf(b, sizeof b, "D m%d S%d F%d o%d%d%d i%d%d f%d a%d%d s%d | %s |", r.mode, r.streams, r.frames, r.s16, r.taps, r.transcode, r.identity,
             r.mix_state, r.fixed, r.acmod, r.lfe, r.src, flags);
    std::string s = b;
    if (err) return s + " refused";
    for (const Launched &k : l) s += " " + k.kernel + " " + std::to_string(k.grid) + "x" + std::to_string(k.block) + ";";
    return s;
}

}  // namespace grid
