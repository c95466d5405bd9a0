// enc_exp.h — the encoder's exponent coding (the reference's encode_exp, ENC/ac3enc.cpp:684-761) wavefront-wide, stated once:
// the +-2 delta constraint over a lane's entries (exp_constrain) and how a lane gets its entries from a row - a channel's
// (chan_exp_entries) or the coupling channel's (cpl_exp_entries).  encode.hip's four routines are these plus what differs
// between them: encode_exp_wave_t / cpl_encode_exp write the row back, encode_exp_sum_t / cpl_exp_sum add the coded exponents
// up for xs_choose.  How many groups a row sends is enc_syntax.h's (syn_exp_groups, syn_cpl_exp_groups); three entries a group.
#pragma once
#include "wave_ops.h"
#include "enc_syntax.h"

namespace ac3mi {

// The constraint: entry i becomes min over the row's entries j of g[j] + 2 |i - j|, a prefix minimum of g[j] - 2 j followed by
// a suffix minimum of g[j] + 2 j - inside the lane first, then ONE scan over the lane totals per direction, carried one lane on.
// g: a lane's N consecutive entries in, constrained out; ix: twice each entry's index; entries that are not `valid` take no
// part (what g holds for them afterwards is not an exponent).  SEEDED (a channel's row): the exponent of bin 0, clamped,
// stands before entry 1 and enters the forward pass as `seed`; the coupling row has nothing before its first entry.
// Returns the head of the suffix scan, wave-uniform: min over j of g[j] + 2 j, what the constraint leaves at index 0.
template <int N, bool SEEDED>
__device__ __forceinline__ int exp_constrain(int (&g)[N], const int (&ix)[N], const bool (&valid)[N], int seed, int lane)
{
    constexpr int INF = 0x3fffffff;
    int t[N];
    t[0] = valid[0] ? g[0] - ix[0] : INF;
#pragma unroll
    for (int c = 1; c < N; c++) {
        const int a = valid[c] ? g[c] - ix[c] : INF;
        t[c] = a < t[c - 1] ? a : t[c - 1];
    }
    {
        int ex = __builtin_amdgcn_update_dpp(INF, wave_incl_scan_min(t[N - 1]), 0x138, 0xf, 0xf, false);        // wave_shr:1
        if (SEEDED) ex = seed < ex ? seed : ex;
#pragma unroll
        for (int c = 0; c < N; c++) g[c] = (t[c] < ex ? t[c] : ex) + ix[c];
    }
    t[N - 1] = valid[N - 1] ? g[N - 1] + ix[N - 1] : INF;
#pragma unroll
    for (int c = N - 2; c >= 0; c--) {
        const int a = valid[c] ? g[c] + ix[c] : INF;
        t[c] = a < t[c + 1] ? a : t[c + 1];
    }
    const int suf = wave_suffix_scan_min(t[0], lane);
    const int ex = __builtin_amdgcn_update_dpp(INF, suf, 0x130, 0xf, 0xf, false);                               // wave_shl:1
#pragma unroll
    for (int c = 0; c < N; c++) g[c] = (t[c] < ex ? t[c] : ex) - ix[c];
    return __builtin_amdgcn_readfirstlane(suf);
}

// the strategy that gives a lane of a channel's row PER entries (D15 4, D25 2, D45 1: syn_grpsize = 4 / PER bins an entry)
template <int PER> constexpr int exp_strategy_of = PER == 4 ? 1 : PER == 2 ? 2 : 3;

// A channel's row, a dword per lane: `own` holds bins 4 lane .. 4 lane + 3, `nxt` the next lane's (only its first byte is
// used; lane 63's lies beyond every ng).  The lane takes bins 4 lane + 1 .. + 4 (bin[]) as PER entries - four for D15, two for
// D25, one for D45: entry i = 1 .. ng is the minimum of bins 1 + (i - 1) gs .. + gs - 1, so no group straddles a lane.  Returns
// the row's bin-0 exponent clamped to 15, the seed of the constraint.
template <int PER>
__device__ __forceinline__ int chan_exp_entries(uint32_t own, uint32_t nxt, int ng, int lane, int (&bin)[4], int (&g)[PER],
                                                int (&ix)[PER], bool (&valid)[PER])
{
    const uint32_t S = __builtin_amdgcn_alignbyte(nxt, own, 1u);
    bin[0] = (int)(S & 0xffu); bin[1] = (int)((S >> 8) & 0xffu); bin[2] = (int)((S >> 16) & 0xffu); bin[3] = (int)(S >> 24);
    const int m01 = bin[1] < bin[0] ? bin[1] : bin[0], m23 = bin[3] < bin[2] ? bin[3] : bin[2];
#pragma unroll
    for (int c = 0; c < PER; c++) {
        g[c] = PER == 4 ? bin[c] : PER == 2 ? (c == 0 ? m01 : m23) : (m23 < m01 ? m23 : m01);
        ix[c] = 2 * (PER * lane + 1 + c);
        valid[c] = PER * lane + 1 + c <= ng;
    }
    const int row0 = (int)(__builtin_amdgcn_readfirstlane((int)own) & 0xff);
    return row0 > 15 ? 15 : row0;
}

// The coupling channel's row in LDS, three entries per lane: entry i = 0 .. ne - 1 is the minimum of bins cs + i gs .. + gs - 1
// (the groups start at cs, whatever its alignment: bytes, not dwords).
__device__ __forceinline__ void cpl_exp_entries(const uint8_t *row, int cs, int ne, int gs, int lane, int (&g)[3], int (&ix)[3],
                                                bool (&valid)[3])
{
    constexpr int INF = 0x3fffffff;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int i = 3 * lane + c;
        ix[c] = 2 * i;
        valid[c] = i < ne;
        int m = INF;
        if (valid[c])
            for (int k = 0; k < gs; k++) { const int e = row[cs + i * gs + k]; m = e < m ? e : m; }
        g[c] = m;
    }
}

}  // namespace ac3mi
