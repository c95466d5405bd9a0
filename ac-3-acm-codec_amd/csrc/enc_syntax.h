// enc_syntax.h — the side information of the frames the encoder writes (A/52 5.3.1-5.3.3 as ENC/ac3enc.cpp:1113-1332 sends
// it, with this encoder's tools), stated once: the field list of the frame header (syn_header) and of an audio block
// (syn_block) over a SINK, the two sinks every build has - SynWriter, the packers' 64-bit field accumulator, and SynCounter,
// which adds widths - and the constant parts of what enc_search_kernel charges a frame for the same fields (syn_priced_fixed,
// syn_priced_cpl; ac3enc.cpp:880-916).
// A sink has put(n, v), flush() and exponents(row, strat, ng): the emitters call the last where a row's absolute exponent
// and its ng 7-bit groups go, and what it does is the sink's (encode.hip: PackSink::exponents; SynCounter: 4 + 7 ng).
// enc_packf_kernel and enc_packb_kernel write through these lists; enc_packb_kernel places its blocks by their closed forms
// (syn_header_bits, syn_block_bits); enc_packf_kernel<FIXED51> without tools places the images of the 5.1 frame
// (syn_block_images_51, syn_header_image_51), a restatement of the lists that tests/syn_images_c holds to them.
// Plain C++: compiles without HIP (tests/enc_syntax_c walks every shape on the host under the sanitisers).
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace ac3mi {

#define SYN_FN __host__ __device__ inline __attribute__((always_inline))

// fixed allocation codes (:861-879) and the coupling leaks, sent with cplleake 1 in block 0
constexpr int sdecaycod = 2, fdecaycod = 1, sgaincod = 1, dbkneecod = 2, floorcod = 4, fgaincod = 4;
constexpr int CPL_FLEAK = 0, CPL_SLEAK = 0;
constexpr int SYN_CPL = -1;             // exponents(): the row of the coupling channel (0..: channel)

// The 64-bit field accumulator.  Side information is wave-uniform: its fields collect in `acc` (scalar registers on the
// device) and reach the frame up to 64 bits at a time through D::store(pos, n, v), n <= 32.  put() has no test per field: at most 64
// bits may collect between two flushes.  The flush points are the emitters' below, and tests/enc_syntax_c checks that bound
// field by field on every shape.  A flush with nothing pending stores nothing and moves nothing.
template <class D>
struct SynWriter {
    uint32_t pos = 0;                   // first bit not yet in the frame
    uint64_t acc = 0;
    int nacc = 0;                       // pending bits, the low `nacc` of acc
    SYN_FN void put(int n, uint32_t v) { acc = (acc << n) | v; nacc += n; }
    SYN_FN void flush()
    {
        if (nacc > 32) {
            static_cast<D *>(this)->store(pos, nacc - 32, (uint32_t)(acc >> 32) & (0xffffffffu >> (64 - nacc)));
            pos += nacc - 32;
            nacc = 32;
        }
        if (nacc > 0) {
            static_cast<D *>(this)->store(pos, nacc, (uint32_t)acc & (0xffffffffu >> (32 - nacc)));
            pos += nacc;
            nacc = 0;
        }
    }
};

struct SynCounter {
    int bits = 0;
    SYN_FN void put(int n, uint32_t) { bits += n; }
    SYN_FN void flush() {}
    SYN_FN void exponents(int, int, int ng) { bits += 4 + 7 * ng; }
};

// ---- the frame header (:1113-1147): syncinfo and BSI, crc1 as zeros ----
// m: the BSI fields as a bsi_word (launch_rule.h), sanitised - the reference's fixed ones are BSI_DEFAULT; compr0 / compr1: the
// compr word of programme 0 / 1, bit 8 = sent (0: compre 0); dual (acmod 0, 1+1): the second programme's dialnorm2 = dialnorm,
// compr2e (+ compr2), langcod2e, audprodi2e.  The MD, DW and dual-mono cases are selected at compile time by VALUE: a kernel
// compiled for one case passes constants (BSI_DEFAULT, 0 for a compr word, its DUAL flag) and the fields fold because every
// function here is always inlined - keep it so; an out-of-line call would turn the packers' constant fields into run-time ones.
template <class K>
SYN_FN void syn_header(K &k, uint32_t fscod, uint32_t frmsizecod, uint32_t bsid, int acmod, bool lfe, bool dual, uint32_t m,
                       uint32_t compr0, uint32_t compr1)
{
    k.put(16, 0x0b77); k.put(16, 0); k.put(2, fscod); k.put(6, frmsizecod); k.put(5, bsid); k.put(3, (m >> 5) & 7u); k.put(3, (uint32_t)acmod);
    k.flush();
    if ((acmod & 1) && acmod != 1) k.put(2, (m >> 8) & 3u);
    if (acmod & 4) k.put(2, (m >> 10) & 3u);
    if (acmod == 2) k.put(2, (m >> 12) & 3u);
    k.put(1, lfe);
    auto programme = [&](uint32_t c) {  // dialnorm, compre (+ compr), langcode, audprodie
        k.put(5, m & 31u);
        if (c & 0x100u) { k.put(1, 1); k.put(8, c & 0xffu); } else k.put(1, 0);
        k.put(2, 0);
    };
    programme(compr0);
    if (dual) programme(compr1);
    k.put(1, (m >> 14) & 1u); k.put(1, (m >> 15) & 1u); k.put(3, 0);      // copyrightb, origbs; timecod1e, timecod2e, addbsie
    k.flush();
}

// ---- an audio block's side information (:1194-1332) ----
struct SynShape {
    int acmod, nfbw, nch;               // nch = nfbw + lfe channels, the LFE last
    bool lfe, dual;
    int nbc;                            // coefficients of an uncoupled full-bandwidth channel
    uint32_t chbwcod;
};
// a frame's coupling: every full-bandwidth channel in coupling, one set of coordinates in block 0, no band merged
struct SynCpl {
    uint32_t word;                      // bit 0 cplinu, bits 8 + 2 ch .. 9 + 2 ch: mstrcplco of channel ch (CplWs::word); 0: none
    int begf, endf;                     // cplbegf, cplendf: bins [37 + 12 begf, 73 + 12 endf), 3 + endf - begf bands
    uint32_t strat;                     // cplexpstr of this block
};

SYN_FN int syn_grpsize(int strat) { return strat == 1 ? 1 : strat == 2 ? 2 : 4; }
// 7-bit groups (three differentials, each held for syn_grpsize bins) behind the absolute exponent: of a channel coding bins
// [0, n), from bin 1 (A/52's nchgrps; nlfegrps at n = 7: the last group may reach beyond n); of the coupling channel over
// [cs, ce), from cs (ncplgrps)
SYN_FN int syn_exp_groups(int n, int strat)
{
    const int gs = syn_grpsize(strat);
    return (n + gs * 3 - 4) / (3 * gs);
}
SYN_FN int syn_cpl_exp_groups(int cs, int ce, int strat) { return (ce - cs) / (3 * syn_grpsize(strat)); }
// rematrixing flags a coupled 2/0 block sends: liba52's band set for cplinu 1
SYN_FN int syn_cpl_nrem(int begf) { return begf == 0 ? 2 : begf <= 2 ? 3 : 4; }

// Block b from blksw to skiple.  Per-row values come as callables: blksw(ch); dynrng(p), programme p's word with bit 8 = sent
// (0: dynrnge 0); strat_of(ch); cplco(ch, band), cplcoexp << 4 | cplcomant.  remat: the 2/0 rematrixing word, rematstr in
// bit 4 over the flags in bits 0-3 (no rematrixing: 0x10 in block 0, 0 after it); a coupled block sends liba52's cplinu-1
// band set of 2, 3 or 4 flags.  csnr, fsnr: block 0's offsets, one fsnroffst for every row.
template <class K, class Blksw, class Dynrng, class Strat, class Cplco>
SYN_FN void syn_block(K &k, const SynShape &s, const SynCpl &c, int b, Blksw blksw, Dynrng dynrng, uint32_t remat, Strat strat_of,
                      Cplco cplco, uint32_t csnr, uint32_t fsnr)
{
    const int nfbw = s.nfbw, nch = s.nch;
    const bool cplf = (c.word & 1u) != 0;
    const int cs = 37 + 12 * c.begf, ce = 73 + 12 * c.endf, ncb = 3 + c.endf - c.begf;
    for (int ch = 0; ch < nfbw; ch++) k.put(1, blksw(ch));
    for (int ch = 0; ch < nfbw; ch++) k.put(1, 1);              // dithflag
    // dynrnge + dynrng, dual mono: dynrng2e + dynrng2 (flushed: the fields up to the first exponent stay within the accumulator)
    auto dynrng_word = [&](uint32_t w) {
        if (w & 0x100u) { k.put(1, 1); k.put(8, w & 0xffu); k.flush(); }
        else k.put(1, 0);
    };
    dynrng_word(dynrng(0));
    if (s.dual) dynrng_word(dynrng(1));
    if (cplf) {
        // cplstre, cplinu, chincpl, phsflginu, cplbegf, cplendf, cplbndstrc (all 0); cplcoe, mstrcplco, the coordinates
        if (b == 0) {
            k.put(1, 1); k.put(1, 1);
            for (int ch = 0; ch < nfbw; ch++) k.put(1, 1);
            if (s.acmod == 2) k.put(1, 0);
            k.put(4, (uint32_t)c.begf); k.put(4, (uint32_t)c.endf); k.put(ncb - 1, 0);
            k.flush();
            for (int ch = 0; ch < nfbw; ch++) {
                k.put(1, 1); k.put(2, (c.word >> (8 + 2 * ch)) & 3u);
                for (int bd = 0; bd < ncb; bd++) { k.put(8, cplco(ch, bd)); if ((bd & 3) == 3) k.flush(); }
                k.flush();
            }
        } else {
            k.put(1, 0);
            for (int ch = 0; ch < nfbw; ch++) k.put(1, 0);
        }
    } else if (b == 0) { k.put(1, 1); k.put(1, 0); } else k.put(1, 0);
    if (s.acmod == 2) {
        const int nrem = cplf ? syn_cpl_nrem(c.begf) : 4;
        k.put(1, remat >> 4);
        if (remat & 0x10u) for (int i = 0; i < nrem; i++) k.put(1, (remat >> i) & 1u);
    }
    if (cplf) k.put(2, c.strat);
    for (int ch = 0; ch < nfbw; ch++) k.put(2, strat_of(ch));
    if (s.lfe) k.put(1, strat_of(nch - 1));
    for (int ch = 0; ch < nfbw; ch++) if (strat_of(ch) != 0 && !cplf) k.put(6, s.chbwcod);
    // exponents: cplabsexp and the groups from cplstrtmant; then each channel's exps[0], its groups from bin 1 and gainrng
    if (cplf && c.strat != 0) k.exponents(SYN_CPL, (int)c.strat, syn_cpl_exp_groups(cs, ce, (int)c.strat));
    for (int ch = 0; ch < nch; ch++) {
        const int stg = (int)strat_of(ch);
        if (stg == 0) continue;
        const bool is_lfe = s.lfe && ch == nch - 1;
        k.exponents(ch, stg, syn_exp_groups(is_lfe ? 7 : cplf ? cs : s.nbc, stg));
        if (!is_lfe) k.put(2, 0);
    }
    if (b == 0) k.flush();
    k.put(1, b == 0);                   // baie
    if (b == 0) { k.put(2, sdecaycod); k.put(2, fdecaycod); k.put(2, sgaincod); k.put(2, dbkneecod); k.put(3, floorcod); }
    k.put(1, b == 0);                   // snroffste
    if (b == 0) {
        k.put(6, csnr);
        if (cplf) { k.put(4, fsnr); k.put(3, fgaincod); k.flush(); }
        for (int ch = 0; ch < nch; ch++) { k.put(4, fsnr); k.put(3, fgaincod); }
    }
    if (cplf) {                         // cplleake (+ cplfleak, cplsleak in block 0)
        k.put(1, b == 0);
        if (b == 0) { k.put(3, CPL_FLEAK); k.put(3, CPL_SLEAK); }
    }
    k.put(1, 0);                        // deltbaie
    k.put(1, 0);                        // skiple
    k.flush();
}

// ---- the same counts in closed form, for an uncoupled frame ----
// enc_packb_kernel places its blocks by these (a wavefront per block: each needs the header's and its own block's bits before
// it writes a field, and the lists on a SynCounter cost it registers it does not have).  tests/enc_syntax_c holds them to the
// lists on every uncoupled shape: a count that differed would land every later block of the frame at the wrong bit.
SYN_FN int syn_header_bits(int acmod, uint32_t compr0, uint32_t compr1)
{
    return 16 + 16 + 2 + 6 + 5 + 3 + 3 + (((acmod & 1) && acmod != 1) ? 2 : 0) + ((acmod & 4) ? 2 : 0) + (acmod == 2 ? 2 : 0) + 1 + 5 + 3 +
           (acmod == 0 ? 8 : 0) + 1 + 1 + 3 + ((compr0 & 0x100u) ? 8 : 0) + ((compr1 & 0x100u) ? 8 : 0);
}
template <class Strat>
SYN_FN int syn_block_bits(const SynShape &s, int b, uint32_t dynrng0, uint32_t dynrng1, uint32_t remat, Strat strat_of)
{
    const int nfbw = s.nfbw, nch = s.nch;
    int bits = 2 * nfbw + 1 + (s.dual ? 1 : 0) + (b == 0 ? 2 : 1) + (s.acmod == 2 ? 1 + ((remat & 0x10u) ? 4 : 0) : 0) + 2 * nfbw + (s.lfe ? 1 : 0) +
               1 + (b == 0 ? 11 : 0) + 1 + (b == 0 ? 6 + 7 * nch : 0) + 2;
    bits += ((dynrng0 & 0x100u) ? 8 : 0) + ((dynrng1 & 0x100u) ? 8 : 0);
    for (int ch = 0; ch < nch; ch++) {
        const int stg = (int)strat_of(ch);
        if (stg == 0) continue;
        const bool is_lfe = s.lfe && ch == nch - 1;
        bits += 4 + 7 * syn_exp_groups(is_lfe ? 7 : s.nbc, stg) + (is_lfe ? 0 : 8);      // (fbw: chbwcod 6 + gainrng 2)
    }
    return bits;
}

// ---- the fixed 5.1 frame once more, as images ----
// A RESTATEMENT for enc_packf_kernel<FIXED51> without tools (acmod 7 + LFE, five full-bandwidth channels, the reference's BSI;
// no coupling, rematrixing, dynrng or compr words): the lists above stay the one authority, and tests/syn_images_c holds
// these to them bit for bit.  Everything between two exponent rows is a constant or a function of the block's six
// strategies, so the block's fields come as two images the lanes OR into the frame and one bit offset per row, instead of
// a field at a time through the accumulator:
//   pre   blksw .. the last chbwcod, MSB-first (bit 31 of pre[0] = the block's first bit), pre_bits <= 54
//   suf   baie .. skiple, suf_bits = 63 in block 0 (the allocation codes and offsets), else 4 zeros; at bit suf_at
//   absexp_at[ch] / gainrng_at[ch]: where a row that sends exponents has its absolute exponent (its groups follow at + 4 + 7 g)
//   and its gainrng (0: the row sends none; the LFE has no gainrng); all offsets from the block's first bit
//   bits  = syn_block_bits
// Values wider than their fields (csnr, fsnr) spill as in the accumulator: onto the fields before them.
struct SynImages51 {
    uint32_t pre[2], suf[2];
    int pre_bits, suf_bits, suf_at, bits;
    int absexp_at[6], gainrng_at[6];
};
// blksw: channel 0's flag in bit 4 .. channel 4's in bit 0; strat_of(ch), ch 5 = the LFE; nbc, chbwcod: SynShape's
template <class Strat>
SYN_FN void syn_block_images_51(SynImages51 &im, int b, uint32_t blksw, Strat strat_of, int nbc, uint32_t chbwcod, uint32_t csnr, uint32_t fsnr)
{
    uint64_t acc = ((uint64_t)blksw << 5) | 31u;                // blksw, dithflag
    acc = b == 0 ? (acc << 3) | 2u : acc << 2;                  // dynrnge 0; cplstre (+ cplinu 0 in block 0)
    int n = b == 0 ? 13 : 12;
    for (int ch = 0; ch < 5; ch++) acc = (acc << 2) | strat_of(ch);
    acc = (acc << 1) | strat_of(5);
    n += 11;
    for (int ch = 0; ch < 5; ch++)
        if (strat_of(ch) != 0) { acc = (acc << 6) | chbwcod; n += 6; }
    im.pre_bits = n;
    acc <<= 64 - n;                                             // (23 <= n <= 54)
    im.pre[0] = (uint32_t)(acc >> 32);
    im.pre[1] = (uint32_t)acc;
    int at = n;
    for (int ch = 0; ch < 6; ch++) {
        const int stg = (int)strat_of(ch);
        im.absexp_at[ch] = im.gainrng_at[ch] = 0;
        if (stg == 0) continue;
        im.absexp_at[ch] = at;
        at += 4 + 7 * syn_exp_groups(ch == 5 ? 7 : nbc, stg);
        if (ch < 5) { im.gainrng_at[ch] = at; at += 2; }
    }
    im.suf_at = at;
    // baie, the five codes, snroffste, csnroffst, six fsnroffst / fgaincod pairs, deltbaie, skiple
    uint64_t s = (1u << 11) | (sdecaycod << 9) | (fdecaycod << 7) | (sgaincod << 5) | (dbkneecod << 3) | floorcod;
    s = (((s << 1) | 1u) << 6) | csnr;
    for (int ch = 0; ch < 6; ch++) s = (((s << 4) | fsnr) << 3) | fgaincod;
    s <<= 3;                                                    // (the two zeros; 63 bits, left-aligned)
    im.suf[0] = b == 0 ? (uint32_t)(s >> 32) : 0u;
    im.suf[1] = b == 0 ? (uint32_t)s : 0u;
    im.suf_bits = b == 0 ? 63 : 4;
    im.bits = at + im.suf_bits;
}
// dword j (0, 1, 2) of what a two-dword image w0 : w1 puts into the frame's MSB-first dwords from dword at >> 5 on, its first
// bit at bit `at`: a funnel shift (v_alignbit_b32) per dword, one lane each
SYN_FN uint32_t syn_image_dword(uint32_t w0, uint32_t w1, int j, uint32_t at)
{
    const uint32_t a = j == 1 ? w0 : j == 2 ? w1 : 0u, c = j == 0 ? w0 : j == 1 ? w1 : 0u, s = at & 31u;
    return s ? (a << (32u - s)) | (c >> s) : c;
}
// The header of the same frames (syn_header with BSI_DEFAULT, acmod 7, LFE, no compr word: 69 bits), crc1 as zeros
constexpr int SYN_HEADER_BITS_51 = 69;
SYN_FN void syn_header_image_51(uint32_t (&w)[3], uint32_t fscod, uint32_t frmsizecod, uint32_t bsid, uint32_t m)
{
    w[0] = 0x0b770000u;
    // fscod 2, frmsizecod 6, bsid 5, bsmod 3, acmod 3 (7), cmixlev 2, surmixlev 2, lfeon 1, dialnorm 5, compre 0, langcode 0 | audprodie 0: 32
    uint32_t v = (fscod << 6) | frmsizecod;
    v = (v << 5) | bsid;
    v = (v << 3) | ((m >> 5) & 7u);
    v = (v << 3) | 7u;
    v = (v << 2) | ((m >> 8) & 3u);
    v = (v << 2) | ((m >> 10) & 3u);
    v = (v << 1) | 1u;
    v = (v << 5) | (m & 31u);
    w[1] = v << 3;
    w[2] = ((((m >> 14) & 1u) << 1) | ((m >> 15) & 1u)) << 30;                 // copyrightb, origbs; timecod1e, timecod2e, addbsie 0
}

// ---- what the SNR-offset search charges a frame besides its channels' exponents and mantissas (:880-916) ----
// The reference's sum with its quirks, which are the search's on purpose (it must decide what the reference decides): it
// counts what follows the blocks too - auxdatae, crcrsv and crc2 - and never block 0's rematrixing flags (2/0).
// enc_search_kernel adds to these, as it finds them in the frame: 8 bits per full-bandwidth channel-block that sends exponents
// (chbwcod, gainrng; 2 when coupled), 8 per dynrng / compr word sent, the flags of blocks 1..5 with rematstr 1 (4, coupled:
// syn_cpl_nrem) and the coupling exponents.  The layout's part, every frame's:
SYN_FN int syn_priced_fixed(int acmod, bool lfe, int nfbw, int nch)
{
    // (dual mono: dialnorm2, compr2e, langcod2e, audprodi2e in the BSI; dynrng2e in every block)
    const int extra[8] = {8, 0, 2, 2, 2, 4, 2, 4};
    int bits = 65 + extra[acmod & 7];
    bits += 6 * (nfbw * 2 + 2 + (acmod == 2 ? 1 : 0) + (acmod == 0 ? 1 : 0) + 2 * nfbw + (lfe ? 1 : 0) + 1 + 1 + 2);
    bits++;
    bits += 2 * 4 + 3 + 6 + nch * (4 + 3);
    bits += 2;
    bits += 16;
    return bits;
}
// ... and of a coupled frame with nb coupling bands: chincpl, phsflginu (2/0), cplbegf / cplendf, cplbndstrc; cplcoe, mstrcplco
// and the coordinates in block 0, cplcoe 0 in blocks 1..5; cplexpstr; cplfsnroffst / cplfgaincod; cplleake (+ the two leaks in
// block 0)
SYN_FN int syn_priced_cpl(int acmod, int nfbw, int nb)
{
    return nfbw + (acmod == 2 ? 1 : 0) + 8 + (nb - 1) + nfbw * (3 + 8 * nb) + 5 * nfbw + 6 * 2 + 7 + 7 + 5;
}
}  // namespace ac3mi
