/* csrc/snr_window.h on the host, for tests/test_snr_window_cpu.py: built without HIP, with -fsanitize=address,undefined, and run
 * on its own (never loaded into Python).
 *   step     every x in -8192..8191, every t in 0..15: max((x - 4 t) >> 5, 0) == k0 - [t >= t1] - [t >= t2]
 *   address  every exponent 0..24 and 255 (a bin the row does not code), the same x and t: the address after the steps taken at t
 *            equals the per-candidate formula's of the three-offset sweep (encode.hip, cost_and_record), as an address and as
 *            the byte offset clamp(term + 4 j - 16 e, 0, 252)
 *   window   frames of random rows (band masks, exponents, the blocks a row covers), costed the window's way - three look-ups a
 *            bin, band sums as differences of prefix sums modulo 2^32, widened, entered into a per-block histogram at the run's
 *            first block and taken back behind its last, summed over blocks and steps - against a count offset by offset with
 *            the per-candidate formula: bits, the three counts, ceilings and sixths of every block at all sixteen offsets.
 *            Among them rows whose k reaches 0 inside the window, an LFE row of 7 bins, windows at lo = 0 and lo = 1008.
 *   rule     win_first_lo / win_next_lo on drawn states: inside 0..1008; printed as `rule ...` lines for the Python restatement
 *   snr_window SEED FRAMES */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "snr_window.h"

using namespace ac3mi;

static uint64_t g_rng;
static uint32_t rnd()
{
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_rng >> 33);
}
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

// A/52 table 7.16 (bap by address) and the plain mantissa widths; the cost word as enc_search_kernel builds it
static const uint8_t kBap[64] = {0, 1, 1, 1, 1, 1, 2, 2, 3, 3, 3, 4, 4, 5, 5, 6, 6, 6, 6, 7, 7, 7, 7, 8, 8, 8, 8, 9, 9, 9, 9, 10,
                                 10, 10, 10, 11, 11, 11, 11, 12, 12, 12, 12, 13, 13, 13, 13, 14, 14, 14, 14, 14, 14, 14, 14, 15, 15, 15, 15, 15, 15, 15, 15, 15};
static int plain_bits(int bp) { return bp == 3 ? 3 : bp == 5 ? 4 : bp == 14 ? 14 : bp == 15 ? 16 : bp >= 6 ? bp - 1 : 0; }
static uint32_t lut(int a)
{
    const int bp = kBap[a];
    return (uint32_t)plain_bits(bp) | ((uint32_t)(bp == 1) << 9) | ((uint32_t)(bp == 2) << 14) | ((uint32_t)(bp == 4) << 19);
}
// A/52 table 7.13: first bin of the fifty bands, and the end of the last
static const int kBandStart[51] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 34, 37, 40,
                                   43, 46, 49, 55, 61, 67, 73, 79, 85, 97, 109, 121, 133, 157, 181, 205, 229, 253};

// the three-offset sweep's address of a bin at one candidate offset: m - snroffset = x
static int old_addr4(int x, int e)
{
    int q = (x >> 3) & ~3;
    q = q < 0 ? 0 : q;
    const int a = 320 - q - 16 * e;
    return a < 0 ? 0 : a > 252 ? 252 : a;
}

static void check_step_and_address()
{
    static const int exps[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 255};
    for (int x = -8192; x <= 8191; x++) {
        int k0, t1, t2;
        win_steps(x, k0, t1, t2);
        CHECK(t1 >= 1 && t1 <= WIN_NEVER && t2 >= 9 && t2 <= WIN_NEVER && (k0 >= 1) == (t1 <= 8) && (k0 >= 2 || t2 == WIN_NEVER), "steps of x=%d: %d %d %d", x, k0, t1, t2);
        for (int t = 0; t < WIN_N; t++) {
            int k = (x - 4 * t) >> 5;
            k = k < 0 ? 0 : k;
            const int j = win_taken(t, t1, t2);
            CHECK(k == k0 - j, "step rule: x=%d t=%d: k=%d, k0=%d t1=%d t2=%d", x, t, k, k0, t1, t2);
            for (int e : exps) {
                const int want = old_addr4(x - 4 * t, e);
                int byte = win_term(k0) + 4 * j - 16 * e;
                byte = byte < 0 ? 0 : byte > 252 ? 252 : byte;
                CHECK(4 * win_addr(k0, j, e) == want && byte == want, "address rule: x=%d t=%d e=%d: %d / %d, want %d", x, t, e, 4 * win_addr(k0, j, e), byte, want);
            }
        }
    }
    for (int g = 0; g < 1024; g++) CHECK(win_snroffset(g) == (g - 240) * 4, "snroffset");
}

struct Row {
    int16_t mask[50];
    uint8_t e[256];         // 255: not coded
    int b_in, b_out;        // the run's blocks [b_in, b_out)
};

struct Totals { uint32_t bits[6], n1[6], n2[6], n4[6], ceil[6], sixths[6]; };

static void brute(const std::vector<Row> &rows, int g, Totals &T)
{
    memset(&T, 0, sizeof T);
    const int so = win_snroffset(g);
    for (const Row &r : rows) {
        uint32_t bits = 0, n1 = 0, n2 = 0, n4 = 0;
        for (int band = 0; band < 50; band++)
            for (int i = kBandStart[band]; i < kBandStart[band + 1]; i++) {
                const int bp = kBap[old_addr4(r.mask[band] - so, r.e[i]) >> 2];
                bits += (uint32_t)plain_bits(bp); n1 += bp == 1; n2 += bp == 2; n4 += bp == 4;
            }
        for (int B = r.b_in; B < r.b_out; B++) { T.bits[B] += bits; T.n1[B] += n1; T.n2[B] += n2; T.n4[B] += n4; }
    }
    for (int B = 0; B < 6; B++) {
        T.ceil[B] = 5 * ((T.n1[B] + 2) / 3) + 7 * ((T.n2[B] + 2) / 3) + 7 * ((T.n4[B] + 1) / 2);
        T.sixths[B] = 6 * T.ceil[B] - (10 * T.n1[B] + 14 * T.n2[B] + 21 * T.n4[B]);
    }
}

// the window's way; returns how many bands reached k = 0 inside the window
static int window(const std::vector<Row> &rows, int lo, Totals (&T)[WIN_N])
{
    uint32_t hist[7][17][2], base[6][2];
    memset(hist, 0, sizeof hist);
    memset(base, 0, sizeof base);
    int floored = 0;
    const int so = win_snroffset(lo);
    for (const Row &r : rows) {
        uint32_t P[3][257];             // prefix sums over the bins, modulo 2^32, started from a value that overflows soon
        for (int c = 0; c < 3; c++) P[c][0] = 0xfffffff0u + (uint32_t)c;
        int k0[50], t1[50], t2[50];
        for (int band = 0; band < 50; band++) {
            win_steps(r.mask[band] - so, k0[band], t1[band], t2[band]);
            const int k15 = (r.mask[band] - so - 60) >> 5;
            floored += k0[band] > 0 && k15 <= 0;
            for (int i = kBandStart[band]; i < kBandStart[band + 1]; i++)
                for (int c = 0; c < 3; c++) P[c][i + 1] = P[c][i] + lut(win_addr(k0[band], c, r.e[i]));
        }
        for (int band = 0; band < 50; band++) {
            uint32_t W[3];
            for (int c = 0; c < 3; c++) W[c] = P[c][kBandStart[band + 1]] - P[c][kBandStart[band]];
            CHECK((W[0] & 0x1ff) <= 384 && (W[0] >> 24) == 0, "a band's sum left its fields");
            for (int B = r.b_in; B < r.b_out; B++) { base[B][0] += win_wide_a(W[0]); base[B][1] += win_wide_b(W[0]); }
            if (t1[band] < WIN_N) {
                hist[r.b_in][t1[band]][0] += win_wide_a(W[1]) - win_wide_a(W[0]); hist[r.b_in][t1[band]][1] += win_wide_b(W[1]) - win_wide_b(W[0]);
                hist[r.b_out][t1[band]][0] -= win_wide_a(W[1]) - win_wide_a(W[0]); hist[r.b_out][t1[band]][1] -= win_wide_b(W[1]) - win_wide_b(W[0]);
            }
            if (t2[band] < WIN_N) {
                hist[r.b_in][t2[band]][0] += win_wide_a(W[2]) - win_wide_a(W[1]); hist[r.b_in][t2[band]][1] += win_wide_b(W[2]) - win_wide_b(W[1]);
                hist[r.b_out][t2[band]][0] -= win_wide_a(W[2]) - win_wide_a(W[1]); hist[r.b_out][t2[band]][1] -= win_wide_b(W[2]) - win_wide_b(W[1]);
            }
        }
    }
    for (int t = 0; t < WIN_N; t++) {
        for (int B = 0; B < 6; B++) {
            uint32_t a = base[B][0], b = base[B][1];
            for (int bb = 0; bb <= B; bb++)
                for (int tt = 0; tt <= t; tt++) { a += hist[bb][tt][0]; b += hist[bb][tt][1]; }
            uint32_t e6;
            const uint32_t bits = win_block_bits(a, b, e6);
            T[t].bits[B] = a & 0x7fff; T[t].n1[B] = a >> 15; T[t].n2[B] = b & 0x7ff; T[t].n4[B] = b >> 11;
            T[t].ceil[B] = bits - (a & 0x7fff); T[t].sixths[B] = e6;
        }
    }
    return floored;
}

// a frame of rows: nch channels (the last an LFE row of 7 bins when lfe), runs of random length over the six blocks
static std::vector<Row> draw_frame(int nch, bool lfe, int level, int spread)
{
    std::vector<Row> rows;
    for (int ch = 0; ch < nch; ch++) {
        const int nb = lfe && ch == nch - 1 ? 7 : rnd_in(0, 3) ? 253 : rnd_in(73, 253);
        for (int b = 0; b < 6;) {
            Row r;
            r.b_in = b;
            r.b_out = b + rnd_in(1, 6 - b);
            for (int band = 0; band < 50; band++) r.mask[band] = (int16_t)(level + rnd_in(-spread, spread));
            const int centre = rnd_in(2, 20);
            for (int i = 0; i < 256; i++) {
                const int e = centre + rnd_in(-3, 4);
                r.e[i] = i < nb ? (uint8_t)(e < 0 ? 0 : e > 24 ? 24 : e) : 255;
            }
            rows.push_back(r);
            b = r.b_out;
        }
    }
    return rows;
}

int main(int argc, char **argv)
{
    g_rng = argc > 1 ? (uint64_t)atoll(argv[1]) : 1;
    const int frames = argc > 2 ? atoi(argv[2]) : 40;
    check_step_and_address();
    printf("step_address ok\n");
    int floored = 0, lfe_rows = 0, checked = 0;
    for (int f = 0; f < frames; f++) {
        const int nch = f % 3 == 0 ? 6 : rnd_in(1, 6);
        const bool lfe = f % 3 == 0 || (rnd() & 1);
        const int lo = f % 5 == 0 ? 0 : f % 5 == 1 ? WIN_LO_MAX : rnd_in(0, WIN_LO_MAX);
        // masks placed so that k is small at the window (some bands reach 0 inside it) or anywhere above
        const int level = win_snroffset(lo) + (f % 2 ? rnd_in(0, 96) : rnd_in(0, 1800)), spread = rnd_in(0, 200);
        const std::vector<Row> rows = draw_frame(nch, lfe, level, spread);
        lfe_rows += lfe;
        Totals W[WIN_N];
        floored += window(rows, lo, W);
        for (int t = 0; t < WIN_N; t++) {
            Totals T;
            brute(rows, lo + t, T);
            for (int B = 0; B < 6; B++) {
                CHECK(T.bits[B] == W[t].bits[B] && T.n1[B] == W[t].n1[B] && T.n2[B] == W[t].n2[B] && T.n4[B] == W[t].n4[B],
                      "frame %d lo %d t %d block %d: counts %u %u %u %u, window %u %u %u %u", f, lo, t, B, T.bits[B], T.n1[B], T.n2[B], T.n4[B],
                      W[t].bits[B], W[t].n1[B], W[t].n2[B], W[t].n4[B]);
                CHECK(T.ceil[B] == W[t].ceil[B] && T.sixths[B] == W[t].sixths[B] && T.sixths[B] <= 69, "frame %d lo %d t %d block %d: ceilings %u / %u, sixths %u / %u",
                      f, lo, t, B, T.ceil[B], W[t].ceil[B], T.sixths[B], W[t].sixths[B]);
                checked++;
            }
        }
    }
    printf("window ok frames=%d checked=%d floored=%d lfe=%d\n", frames, checked, floored, lfe_rows);
    // the rule on drawn states
    for (int i = 0; i < 4000; i++) {
        const int hint = rnd() & 1 ? rnd_in(1, 1023) : 0, cold = (int)(rnd() & 1), g_prev = rnd_in(0, 1023);
        const int first = win_first_lo(hint, cold != 0, g_prev);
        int gl = rnd() % 4 ? rnd_in(0, 1023) : -1, gh = rnd() % 4 ? rnd_in(0, 1023) : -1;
        if (gl < 0 && gh < 0) gl = rnd_in(0, 1023);
        const int sl = rnd_in(0, 30000), sh = -rnd_in(1, 30000), slope = rnd_in(-50, 4000), sweeps = rnd_in(1, 9), gq = rnd_in(0, 1023);
        const int cmin = rnd_in(0, WIN_LO_MAX), cspan = cmin + 15 + 16 * rnd_in(0, 3), cmax = cspan > 1023 ? 1023 : cspan;
        const int next = win_next_lo(sweeps, gl, sl, gh, sh, slope, cmin, cmax, gq);
        CHECK(first >= 0 && first <= WIN_LO_MAX && next >= 0 && next <= WIN_LO_MAX, "rule: a window outside 0..1008");
        if (sweeps >= WIN_ASK_SWEEPS) CHECK(next <= gq && gq < next + WIN_N, "rule: the late window misses the question");
        printf("rule %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", hint, cold, g_prev, first, sweeps, gl, sl, gh, sh, slope, cmin, cmax, gq, next);
    }
    return 0;
}
