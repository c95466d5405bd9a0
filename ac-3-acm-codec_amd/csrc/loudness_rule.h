// loudness_rule.h — the parts of the BS.1770 meter (ac3mi_loudness_*, include/ac3mi.h) that need no GPU: the state's layout,
// the frozen K-weighting coefficients, the bin-edge and dialnorm tables, and the three decisions - a block's bin, the gated
// read-out of the bins, the dialnorm word - as __host__ __device__ functions that loudness_kernel / loudness_read_kernel
// (loudness.hip) and the host twin ac3mi_loudness_read both call.  No decision uses a logarithm: blocks and means are
// compared as energies against tables built once on the host in double.  Behind it the same for the loudness range meter
// (ac3mi_loudness_range_*, EBU Tech 3342): RangeState, the one step that advances it, and the percentile read-out.
// Plain C++: compiles without HIP (a host-only build of loudness.hip for the sanitiser programs of tests/loudness_c and
// tests/loudness_range_c).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "../../include/ac3mi.h"

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace ac3mi {

constexpr int LOUD_BINS = 900;          // 0.1 LU each over [-70, +20) LKFS
constexpr int LOUD_SEG = 24;            // sample instants a lane owns in a frame: 64 x 24 = 1536

// One stream's state (ac3mi_loudness_state_bytes() = sizeof): all zeros is a new stream.
struct LoudState {
    double bq[6][4];                    // per input slot: shelf s1, s2, high-pass s1, s2 (transposed direct form II)
    double hop_sum;                     // the open hop's energy so far
    double hops[3];                     // the last three closed hops, oldest first
    double max_block;                   // the largest block energy z seen
    uint32_t pos;                       // samples in the open hop
    uint32_t hop_count;                 // closed hops (a block per hop from the fourth on)
    uint32_t blocks, blocks_abs;        // blocks formed, and those at or above the absolute gate
    uint32_t count[LOUD_BINS];          // per bin: the blocks in it
    double sum[LOUD_BINS];              // ... and their energies, added in time order
};
static_assert(sizeof(LoudState) == 11048 && offsetof(LoudState, sum) % 8 == 0, "LoudState layout");

// K-weighting, frozen: shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2 (a0 = 1) from the bilinear design of include/ac3mi.h,
// evaluated in double; the 48 kHz row is BS.1770's table to its printed digits.  nullptr: not a rate the meter takes
inline const double *loud_coefs(int sample_rate)
{
    static const double C48[10] = {1.5351248595869702, -2.6916961894063807, 1.19839281085285, -1.6906592931824103, 0.7324807742158501,
                                   1.0, -2.0, 1.0, -1.9900474548339797, 0.9900722503662099};
    static const double C44[10] = {1.5308412300503478, -2.6509799951547297, 1.169079079921587, -1.6636551132560204, 0.7125954280732254,
                                   1.0, -2.0, 1.0, -1.989169673629796, 0.9891990357870393};
    static const double C32[10] = {1.5111778995687646, -2.464889413360141, 1.0416332735222955, -1.5390450962506403, 0.626966855981559,
                                   1.0, -2.0, 1.0, -1.9850896689886883, 0.9851453206695515};
    return sample_rate == 48000 ? C48 : sample_rate == 44100 ? C44 : sample_rate == 32000 ? C32 : nullptr;
}

// E_b = 10^((-70 + 0.1 b + 0.691) / 10), b = 0..900: bin b holds the blocks with E_b <= z < E_(b+1)
inline void loud_build_edges(double *edges901)
{
    for (int b = 0; b <= LOUD_BINS; b++) edges901[b] = pow(10.0, (-70.0 + 0.1 * b + 0.691) / 10.0);
}

// T_d = 10^((-d - 0.5 + 0.691) / 10) at [d - 1], d = 1..30: a mean below T_d is quieter than -(d + 0.5) LKFS
inline void loud_build_dialnorm(double *thr30)
{
    for (int d = 1; d <= 30; d++) thr30[d - 1] = pow(10.0, (-d - 0.5 + 0.691) / 10.0);
}

// The cascade as a linear system on v = (s1, s2, t1, t2): v' = A v + B x, y = C v + D x with
//   y1 = b0 x + s1, s1' = b1 x - a1 y1 + s2, s2' = b2 x - a2 y1;  y = y1 + t1, t1' = -2 y1 - c1 y + t2, t2' = y1 - c2 y.
// For the segmented kernel: M[k] = A^(24 2^k) (row-major 4 x 4, k = 0..5) and Z[n] = C A^n (n = 0..23), the zero-input response.
inline void loud_build_segment(const double *coef, double M[6][16], double Z[LOUD_SEG][4])
{
    const double a1 = coef[3], a2 = coef[4], c1 = coef[8], c2 = coef[9];
    const double A[16] = {-a1, 1, 0, 0, -a2, 0, 0, 0, -2 - c1, 0, -c1, 1, 1 - c2, 0, -c2, 0};
    auto mul = [](const double *x, const double *y, double *o) {
        double t[16];
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) t[4 * r + c] = x[4 * r] * y[c] + x[4 * r + 1] * y[4 + c] + x[4 * r + 2] * y[8 + c] + x[4 * r + 3] * y[12 + c];
        memcpy(o, t, sizeof t);
    };
    double P[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};      // A^n
    for (int n = 0; n < LOUD_SEG; n++) {
        for (int c = 0; c < 4; c++) Z[n][c] = P[c] + P[8 + c];              // C = (1, 0, 1, 0)
        mul(A, P, P);
    }
    memcpy(M[0], P, sizeof P);
    for (int k = 1; k < 6; k++) mul(M[k - 1], M[k - 1], M[k]);
}

// A block's bin: -1 below the absolute gate (z < E_0, or not a number), else the b with E_b <= z < E_(b+1), 899 from E_900 on
__host__ __device__ inline int loud_bin(const double *edges, double z)
{
    if (!(z >= edges[0])) return -1;
    int lo = 0, hi = LOUD_BINS;                         // edges[lo] <= z, and the answer is below hi
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (z >= edges[mid]) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Read-out, first pass: the sums and counts of bins first, first + stride, ... (the host: 0 and 1; a lane: itself and 64)
__host__ __device__ inline void loud_total_part(const LoudState *st, int first, int stride, double *sum, uint32_t *count)
{
    double s = 0;
    uint32_t n = 0;
    for (int b = first; b < LOUD_BINS; b += stride) {
        s += st->sum[b];
        n += st->count[b];
    }
    *sum = s;
    *count = n;
}

// The relative gate: -10 LU under the mean of everything above the absolute gate (no such block: 0, and no bin has blocks)
__host__ __device__ inline double loud_gamma(double sum, uint32_t count) { return count ? 0.1 * (sum / (double)count) : 0.0; }

// ... a bin counts whole if its lower edge is at or above the gate; the one bin the gate cuts counts whole iff its own mean
// is at or above the gate; every other bin is out
__host__ __device__ inline bool loud_bin_included(const LoudState *st, const double *edges, int b, double gamma)
{
    const uint32_t n = st->count[b];
    if (!n) return false;
    if (edges[b] >= gamma) return true;
    if (edges[b + 1] > gamma) return st->sum[b] / (double)n >= gamma;
    return false;
}

// ... second pass: the same walk over the bins that count
__host__ __device__ inline void loud_gated_part(const LoudState *st, const double *edges, double gamma, int first, int stride,
                                                double *sum, uint32_t *count)
{
    double s = 0;
    uint32_t n = 0;
    for (int b = first; b < LOUD_BINS; b += stride)
        if (loud_bin_included(st, edges, b, gamma)) {
            s += st->sum[b];
            n += st->count[b];
        }
    *sum = s;
    *count = n;
}

// round-half-up of -lkfs, clamped to 1..31, decided on energies: 1 + the number of d in 1..30 with mean < T_d
__host__ __device__ inline int loud_dialnorm(const double *thr30, double mean_energy)
{
    int dn = 1;
    for (int d = 0; d < 30; d++) dn += mean_energy < thr30[d] ? 1 : 0;
    return dn;
}

// ... and the record, from the gated totals and the state's counters
__host__ __device__ inline void loud_result(const LoudState *st, const double *thr30, double sum, uint32_t count, ac3mi_loudness_result *out)
{
    ac3mi_loudness_result r;
    r.max_block_energy = st->max_block;
    r.blocks = st->blocks;
    r.blocks_abs = st->blocks_abs;
    r.blocks_rel = count;
    for (int i = 0; i < 6; i++) r.reserved[i] = 0;
    if (count) {
        r.mean_energy = sum / (double)count;
        r.lkfs = (float)(-0.691 + 10.0 * log10(r.mean_energy));
        r.dialnorm = (uint8_t)loud_dialnorm(thr30, r.mean_energy);
        r.flags = 0;
    } else {
        r.mean_energy = 0.0;
        r.lkfs = -70.0f;
        r.dialnorm = 31;
        r.flags = AC3MI_LOUDNESS_EMPTY;
    }
    *out = r;
}

// The whole read-out on a state in host memory (any alignment)
inline void loudness_read_host(const void *h_state, ac3mi_loudness_result *out)
{
    static const struct Tables {
        double edges[LOUD_BINS + 1], thr[30];
        Tables() { loud_build_edges(edges); loud_build_dialnorm(thr); }
    } T;
    LoudState *st = new LoudState;
    memcpy(st, h_state, sizeof *st);
    double s;
    uint32_t n;
    loud_total_part(st, 0, 1, &s, &n);
    const double gamma = loud_gamma(s, n);
    loud_gated_part(st, T.edges, gamma, 0, 1, &s, &n);
    loud_result(st, T.thr, s, n, out);
    delete st;
}

// ---- the loudness range meter (ac3mi_loudness_range_*, EBU Tech 3342; the rule is include/ac3mi.h's): a second consumer of
// the closed hop energies.  One stream's state (ac3mi_loudness_range_state_bytes() = sizeof): all zeros is a new stream.
constexpr int RANGE_HOPS = 30;          // hops in a 3 s block
constexpr int RANGE_LANES = 60;         // lanes of the read-out that own bins ...
constexpr int RANGE_RUN = 15;           // ... this many each, one behind the other: 60 x 15 = 900

struct RangeState {
    double ring[RANGE_HOPS];            // ring[k]: the closed hop that was written at ring position k
    double sum_abs;                     // the sum of z3 over the blocks at or above the absolute gate, added in time order
    double max_short;                   // the largest short-term block energy z3 seen
    uint32_t hops;                      // closed hops this state has seen, saturating (a block per hop from the 30th on)
    uint32_t ring_pos;                  // 0..29, where the next closed hop goes (read modulo 30: garbage can only give wrong numbers)
    uint32_t blocks, blocks_abs;        // 3 s blocks formed, and those at or above the absolute gate
    uint32_t count[LOUD_BINS];          // per bin: the blocks in it
};
static_assert(sizeof(RangeState) == 3872 && offsetof(RangeState, count) == 272, "RangeState layout");
static_assert(RANGE_LANES * RANGE_RUN == LOUD_BINS && RANGE_LANES <= 64, "the read-out's runs cover the bins");

// A hop of energy h has closed: into the ring, and from the 30th on the 3 s block behind it - its 30 hops added oldest first,
// one addition after the other (the order is the rule's: the same bits for every way of cutting a stream into calls) - into
// the bins and counters.  block_samples = 30 hop.  The one place the state changes; plain loads and stores
__host__ __device__ inline void range_push_hop(RangeState *rs, const double *edges, double h, double block_samples)
{
    const uint32_t pos = rs->ring_pos % (uint32_t)RANGE_HOPS;
    uint32_t hops = rs->hops;
    if (hops != 0xffffffffu) hops++;
    rs->hops = hops;
    rs->ring[pos] = h;
    rs->ring_pos = pos + 1 == (uint32_t)RANGE_HOPS ? 0 : pos + 1;
    if (hops < (uint32_t)RANGE_HOPS) return;
    double s = 0.0;                     // oldest first: the entry behind pos is the oldest, pos itself the hop just closed
    for (int k = 1; k <= RANGE_HOPS; k++) {
        const uint32_t i = pos + (uint32_t)k;
        const double v = rs->ring[i >= (uint32_t)RANGE_HOPS ? i - RANGE_HOPS : i];
        s = k == 1 ? v : s + v;
    }
    const double z3 = s / block_samples;
    rs->blocks += 1;
    if (z3 > rs->max_short) rs->max_short = z3;
    const int b = loud_bin(edges, z3);
    if (b >= 0) {
        rs->blocks_abs += 1;
        rs->sum_abs += z3;
        rs->count[b] += 1;
    }
}

// Read-out.  The relative gate: -20 LU under the mean of the blocks above the absolute gate (no such block: 0)
__host__ __device__ inline double range_gamma(double sum_abs, uint32_t blocks_abs) { return blocks_abs ? 0.01 * (sum_abs / (double)blocks_abs) : 0.0; }

// ... a bin counts, whole, iff it has blocks and its upper edge lies above the gate (so the one bin the gate cuts counts)
__host__ __device__ inline bool range_bin_included(const RangeState *rs, const double *edges, int b, double gamma)
{
    return rs->count[b] != 0 && edges[b + 1] > gamma;
}

// ... what bin b adds to the counted blocks: its count, or 0
__host__ __device__ inline uint32_t range_counted(const RangeState *rs, const double *edges, int b, double gamma)
{
    return range_bin_included(rs, edges, b, gamma) ? rs->count[b] : 0;
}

// ... the blocks counted in a part of n bins, c[k] = range_counted of the part's k-th bin (the host: all 900; lane l: the 15
// from 15 l on, in registers)
__host__ __device__ inline uint64_t range_counted_sum(const uint32_t *c, int n)
{
    uint64_t t = 0;
    for (int k = 0; k < n; k++) t += c[k];
    return t;
}

// ... the 0-based rank, ascending, of the pct-th percentile among n >= 1 counted blocks: (n - 1) pct / 100 + 0.5, truncated
__host__ __device__ inline uint64_t range_rank(uint64_t n, uint32_t pct) { return ((uint64_t)pct * (n - 1) + 50) / 100; }

// ... the bin that holds the counted block of that rank, if it is one of the part's n bins from bin `first` on, `before`
// blocks being counted in the bins below: the smallest b whose cumulative counted count exceeds rank; -1: not in this part
__host__ __device__ inline int range_bin_of_rank(const uint32_t *c, int first, int n, uint64_t before, uint64_t rank)
{
    int found = -1;
    uint64_t t = before;
    for (int k = 0; k < n; k++) {
        const bool here = found < 0 && t <= rank && t + c[k] > rank;
        found = here ? first + k : found;
        t += c[k];
    }
    return found;
}

// ... a bin's centre in LKFS, -70 + 0.1 b + 0.05, as one division of integers (the same float wherever it is evaluated)
__host__ __device__ inline float range_bin_lkfs(int b) { return (float)((double)(10 * b - 6995) / 100.0); }

// ... and the record, from the counted total and the two bins (low_bin, high_bin: anything when n == 0)
__host__ __device__ inline void range_result(const RangeState *rs, uint64_t n, int low_bin, int high_bin, ac3mi_loudness_range_result *out)
{
    ac3mi_loudness_range_result r;
    const double m = rs->max_short;
    r.max_short_energy = m;
    r.max_short_lkfs = m > 0.0 ? (float)(-0.691 + 10.0 * log10(m)) : -200.0f;
    r.blocks = rs->blocks;
    r.blocks_abs = rs->blocks_abs;
    r.blocks_rel = n > 0xffffffffu ? 0xffffffffu : (uint32_t)n;         // (more than a state's counters can hold: garbage)
    for (int i = 0; i < 5; i++) r.reserved[i] = 0;
    if (n == 0 || low_bin < 0 || high_bin < low_bin) low_bin = high_bin = 0;
    r.low_bin = (uint16_t)low_bin;
    r.high_bin = (uint16_t)high_bin;
    r.lra_tenths = (uint16_t)(high_bin - low_bin);
    r.lra = 0.1f * (float)r.lra_tenths;
    r.low_lkfs = n ? range_bin_lkfs(low_bin) : -70.0f;
    r.high_lkfs = n ? range_bin_lkfs(high_bin) : -70.0f;
    r.flags = n ? 0 : AC3MI_LOUDNESS_RANGE_EMPTY;
    *out = r;
}

// The whole read-out on a state in host memory (any alignment)
inline void loudness_range_read_host(const void *h_range_state, ac3mi_loudness_range_result *out)
{
    static const struct Edges {
        double e[LOUD_BINS + 1];
        Edges() { loud_build_edges(e); }
    } T;
    RangeState *rs = new RangeState;
    memcpy(rs, h_range_state, sizeof *rs);
    const double gamma = range_gamma(rs->sum_abs, rs->blocks_abs);
    uint32_t *c = new uint32_t[LOUD_BINS];
    for (int b = 0; b < LOUD_BINS; b++) c[b] = range_counted(rs, T.e, b, gamma);
    const uint64_t n = range_counted_sum(c, LOUD_BINS);
    int lo = 0, hi = 0;
    if (n) {
        lo = range_bin_of_rank(c, 0, LOUD_BINS, 0, range_rank(n, 10));
        hi = range_bin_of_rank(c, 0, LOUD_BINS, 0, range_rank(n, 95));
    }
    delete[] c;
    range_result(rs, n, lo, hi, out);
    delete rs;
}

}  // namespace ac3mi
