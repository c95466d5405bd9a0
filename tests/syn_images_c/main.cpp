/* csrc/enc_syntax.h's images of the fixed 5.1 frame (syn_block_images_51, syn_image_dword, syn_header_image_51) against the
 * field lists they restate, for tests/test_syn_images_cpu.py: built without HIP, with -fsanitize=address,undefined, and run on
 * its own (never loaded into Python).
 * A case is a frame: 36 strategies, blksw flags, chbwcod (nbc = 73 + 3 chbwcod), csnr, fsnr.  Each of its six blocks is written
 * twice at the same bit `at` of a zeroed buffer, at % 32 in {0, 1, 31}:
 *   - by syn_block through HostSink, the accumulator over a byte buffer, whose exponents() writes a row as absolute exponent 9
 *     and groups of 0x55 and notes where the row and its gainrng went;
 *   - from the images: prefix and suffix as three dwords each (syn_image_dword), the same row pattern at absexp_at + 4 + 7 g.
 * The two buffers must be equal byte for byte, the offsets equal to the notes, `bits` to what the sink moved and to
 * syn_block_bits; the header image to syn_header.  A difference is reported on stderr and ends the run with status 1.
 * The frames: every strategy assignment of one channel over the six blocks (3 x 4^5; the LFE 2^5) for each of the six
 * channels, the other rows D15 in block 0 and reused after it, the six pairs of csnr 0 / 15 / 63 x fsnr 0 / 15 taken in turn;
 * all rows new in all blocks (per strategy) and in block 0 alone, with every pair.  Prints "frames=N blocks=M".
 *   syn_images */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "launch_rule.h"
#include "enc_syntax.h"

using namespace ac3mi;

static long g_frames = 0, g_blocks = 0;
constexpr int BUF = 512;             // bytes: a block is at most 2 755 bits, its first bit below 352

struct HostSink : SynWriter<HostSink> {
    uint8_t buf[BUF];
    int absexp_at[6], gainrng_at[6], after_row = -1;
    HostSink(uint32_t at) { memset(buf, 0, sizeof buf); memset(absexp_at, 0, sizeof absexp_at); memset(gainrng_at, 0, sizeof gainrng_at); pos = at; }
    void put(int n, uint32_t v)
    {
        if (nacc + n > 64) { fprintf(stderr, "frame %ld: more than 64 bits pending\n", g_frames); exit(1); }
        if (after_row >= 0) { gainrng_at[after_row] = (int)pos + nacc; after_row = -1; }
        SynWriter<HostSink>::put(n, v);
    }
    void store(uint32_t at, int n, uint32_t v)
    {
        for (int i = 0; i < n; i++) {
            const uint32_t p = at + (uint32_t)i;
            if (p >= 8 * sizeof buf) { fprintf(stderr, "frame %ld: bit %u beyond the buffer\n", g_frames, p); exit(1); }
            buf[p >> 3] |= (uint8_t)(((v >> (n - 1 - i)) & 1u) << (7 - (p & 7u)));
        }
    }
    void exponents(int row, int, int ng)
    {
        absexp_at[row] = (int)pos + nacc;
        put(4, 9);
        flush();
        for (int g = 0; g < ng; g++) store(pos + 7u * (uint32_t)g, 7, 0x55);
        pos += 7u * (uint32_t)ng;
        after_row = row < 5 ? row : -1;
    }
};

// MSB-first dwords, as the packers' frame in LDS
struct DwordFrame {
    uint32_t w[BUF / 4];
    DwordFrame() { memset(w, 0, sizeof w); }
    void or_dword(uint32_t i, uint32_t v)
    {
        if (i >= BUF / 4) { if (v) { fprintf(stderr, "frame %ld: dword %u beyond the buffer\n", g_frames, i); exit(1); } return; }
        w[i] |= v;
    }
    void image(uint32_t w0, uint32_t w1, uint32_t at) { for (int j = 0; j < 3; j++) or_dword((at >> 5) + (uint32_t)j, syn_image_dword(w0, w1, j, at)); }
    void field(uint32_t at, int n, uint32_t v) { image(v << (32 - n), 0u, at); }
    void compare(const uint8_t *list, int b, uint32_t at) const;
};

struct Frame {
    uint32_t strat[6][6], bsw[6], chbwcod, csnr, fsnr;
};

static void fail(const char *what, int b, uint32_t at, long a, long c)
{
    fprintf(stderr, "frame %ld block %d at bit %u: %s: %ld against %ld\n", g_frames, b, at, what, a, c);
    exit(1);
}

void DwordFrame::compare(const uint8_t *list, int b, uint32_t at) const
{
    uint8_t bytes[BUF];
    for (int i = 0; i < BUF; i++) bytes[i] = (uint8_t)(w[i >> 2] >> (24 - 8 * (i & 3)));
    if (!memcmp(bytes, list, BUF)) return;
    for (int i = 0; i < BUF; i++)
        if (bytes[i] != list[i]) fail("byte differs (index; image << 8 | list)", b, at, i, ((long)bytes[i] << 8) | list[i]);
}

static void run(const Frame &f)
{
    static const uint32_t starts[3] = {0u, 1u, 31u};
    const int nbc = 73 + 3 * (int)f.chbwcod;
    const SynShape shape{7, 5, 6, true, false, nbc, f.chbwcod};
    for (int pi = 0; pi < 3; pi++) {
        for (int b = 0; b < 6; b++) {
            const uint32_t at = 64u * (uint32_t)b + starts[pi];
            auto strat_of = [&](int ch) { return f.strat[b][ch]; };
            HostSink k(at);
            syn_block(k, shape, SynCpl{0u, 0, 12, 0u}, b, [&](int ch) { return (f.bsw[b] >> (4 - ch)) & 1u; }, [](int) { return 0u; },
                      b == 0 ? 0x10u : 0u, strat_of, [](int, int) { return 0u; }, f.csnr, f.fsnr);
            if (k.nacc != 0) fail("bits left pending", b, at, k.nacc, 0);
            SynImages51 im;
            syn_block_images_51(im, b, f.bsw[b], strat_of, nbc, f.chbwcod, f.csnr, f.fsnr);
            DwordFrame d;
            d.image(im.pre[0], im.pre[1], at);
            d.image(im.suf[0], im.suf[1], at + (uint32_t)im.suf_at);
            for (int ch = 0; ch < 6; ch++) {
                const int stg = (int)f.strat[b][ch];
                if (stg == 0) {
                    if (im.absexp_at[ch] != 0 || im.gainrng_at[ch] != 0) fail("offsets of a row that sends nothing", b, at, im.absexp_at[ch], im.gainrng_at[ch]);
                    continue;
                }
                const int ng = syn_exp_groups(ch == 5 ? 7 : nbc, stg);
                const uint32_t r = at + (uint32_t)im.absexp_at[ch];
                if ((int)r != k.absexp_at[ch]) fail("absolute exponent", b, at, (long)r, k.absexp_at[ch]);
                d.field(r, 4, 9);
                for (int g = 0; g < ng; g++) d.field(r + 4u + 7u * (uint32_t)g, 7, 0x55);
                if (ch < 5) {
                    if ((int)at + im.gainrng_at[ch] != k.gainrng_at[ch]) fail("gainrng", b, at, (long)at + im.gainrng_at[ch], k.gainrng_at[ch]);
                    if (im.gainrng_at[ch] != im.absexp_at[ch] + 4 + 7 * ng) fail("gainrng behind the last group", b, at, im.gainrng_at[ch], im.absexp_at[ch] + 4 + 7 * ng);
                } else if (im.gainrng_at[ch] != 0) fail("the LFE has no gainrng", b, at, im.gainrng_at[ch], 0);
            }
            if (at + (uint32_t)im.bits != k.pos) fail("block length against the sink", b, at, im.bits, (long)(k.pos - at));
            if (im.bits != syn_block_bits(shape, b, 0u, 0u, b == 0 ? 0x10u : 0u, strat_of)) fail("block length against syn_block_bits", b, at, im.bits, 0);
            if (im.suf_at + im.suf_bits != im.bits || im.pre_bits > 64 || im.suf_bits > 64) fail("image lengths", b, at, im.pre_bits, im.suf_bits);
            if (im.pre_bits < 64 && ((((uint64_t)im.pre[0] << 32) | im.pre[1]) << im.pre_bits) != 0) fail("prefix bits behind its length", b, at, im.pre_bits, 0);
            if (((((uint64_t)im.suf[0] << 32) | im.suf[1]) << im.suf_bits) != 0) fail("suffix bits behind its length", b, at, im.suf_bits, 0);
            d.compare(k.buf, b, at);
            g_blocks++;
        }
    }
    g_frames++;
}

static void header()
{
    for (uint32_t fscod = 0; fscod < 3; fscod++)
        for (uint32_t frmsizecod = 0; frmsizecod < 38; frmsizecod++)
            for (uint32_t bsid = 6; bsid <= 8; bsid += 2) {
                HostSink k(0u);
                syn_header(k, fscod, frmsizecod, bsid, 7, true, false, BSI_DEFAULT, 0u, 0u);
                uint32_t w[3];
                syn_header_image_51(w, fscod, frmsizecod, bsid, BSI_DEFAULT);
                if (k.nacc != 0 || k.pos != (uint32_t)SYN_HEADER_BITS_51 || SYN_HEADER_BITS_51 != syn_header_bits(7, 0u, 0u)) fail("header length", -1, 0u, k.pos, SYN_HEADER_BITS_51);
                DwordFrame d;
                for (uint32_t j = 0; j < 3; j++) d.or_dword(j, w[j]);
                d.compare(k.buf, -1, 0u);
            }
}

int main(int argc, char **)
{
    if (argc != 1) return 2;
    header();
    static const uint32_t csnrs[3] = {0u, 15u, 63u}, fsnrs[2] = {0u, 15u};
    long n = 0;
    Frame f;
    auto base = [&](int pair) {
        memset(&f, 0, sizeof f);
        f.csnr = csnrs[pair % 3]; f.fsnr = fsnrs[pair / 3];
        f.chbwcod = (n % 3) == 2 ? 30u : 50u;           // (the bandwidth tool's run-time nbc: 163 bins)
        for (int b = 0; b < 6; b++) f.bsw[b] = (uint32_t)((n * 7 + b * 11) % 32) * (uint32_t)(n % 2);
        n++;
    };
    // one channel's strategies over the six blocks, the others D15 in block 0 and reused after it
    for (int ch = 0; ch < 6; ch++) {
        const int opts = ch == 5 ? 2 : 4, first = ch == 5 ? 1 : 3;
        int total = first;
        for (int b = 1; b < 6; b++) total *= opts;
        for (int code = 0; code < total; code++) {
            base((int)(n % 6));
            for (int c2 = 0; c2 < 6; c2++) f.strat[0][c2] = 1u;
            int c = code;
            f.strat[0][ch] = 1u + (uint32_t)(c % first); c /= first;
            for (int b = 1; b < 6; b++) { f.strat[b][ch] = (uint32_t)(c % opts); c /= opts; }
            run(f);
        }
    }
    // all six channels: new sets in every block, per strategy (the LFE D15); block 0 alone
    for (int pair = 0; pair < 6; pair++)
        for (uint32_t s = 1; s <= 3; s++) {
            base(pair);
            for (int b = 0; b < 6; b++)
                for (int ch = 0; ch < 6; ch++) f.strat[b][ch] = ch == 5 ? 1u : s;
            run(f);
            base(pair);
            for (int ch = 0; ch < 6; ch++) f.strat[0][ch] = ch == 5 ? 1u : s;
            run(f);
        }
    printf("frames=%ld blocks=%ld\n", g_frames, g_blocks);
    return 0;
}
