// dec_syntax.h — the side information of the frames the decoder reads (A/52 5.3.2-5.3.3 as liba52 reads it, L52/parse.c:131-205,
// 572-772, 800-804), stated once: the field list of a52_frame behind the sync-rule test (dsyn_frame), of an audio block's first
// half, blksw to the exponent fields (dsyn_block_a), of its second half, baie to deltba (dsyn_block_b), and the skip field
// (dsyn_skip_field).  Both front ends read through these lists - decode_kernel (decode_kernel.h) calls them back to back, with
// its bit allocation between the third and the fourth; decode_wg_kernel's parser wavefront (decode_wg.hip) calls them where its
// workgroup barriers cut the block - and each supplies three things:
//   a reader R   get(n), sget(n), pos(), skip(n): Rd (decode_common.h), VRd (decode_wg.hip)
//   a state S    a52_state_t's side-information fields (L52/a52_internal.h:35-88) behind accessors name() / set_name(v), the
//                slots' endm / cbai / deltbae by index (0..4 full-bandwidth channels, 5 LFE - deltbae: coupling -, 6 coupling
//                channel): St (decode_common.h, packed in scalar registers), PView (decode_wg.hip, ParserState in LDS)
//   a sink K     what differs by kernel:
//                  dynrng(code, programme, apply) -> the word's range factor where apply (the raw word is the sink's to keep)
//                  cplco(ch, band, exponent, mantissa, master), cplco_flip(band): a coupling coordinate, channel 1's sign
//                  exponents(slot, strategy, groups, absolute exponent, first bin, bit position) -> 1 on error: an exponent
//                    field - decode_kernel reads the groups there, decode_wg_kernel records the position for its channel waves
//                  deltba_clear(slot), deltba_seg(slot, band, len, delta): a delta bit allocation row and one segment of it
//                  lap(point): measurement builds' time stamps (0 behind dynrng, 1 behind rematflg, 2 ahead of the exponents)
// The lists return 1 where liba52 refuses the block (acmod < 2 coupled, cplendf + 3 - cplbegf < 0, chbwcod > 60, a deltba
// segment that reaches band 50) or the sink reports an exponent error; state set up to there stays set, as in liba52.
// Results computed from parsed state (gains, the all-zero test, sub-band -> band, descriptors, taps) are the kernels'.
// State, reader and sink go by reference into always-inlined functions: keep it so - a closure or an out-of-line call that
// holds a state's address puts the whole state into scratch.
// Plain C++: compiles without HIP (tests/dec_syntax_c walks frames on the host under the sanitisers against tests/ac3_syntax.py).
#pragma once
#include <stdint.h>
#include "a52_levels.h"

namespace ac3mi {

#define DSYN_FN __host__ __device__ inline __attribute__((always_inline))
#if defined(__clang__)
#define DSYN_UNROLL _Pragma("unroll")
#else
#define DSYN_UNROLL
#endif

// ---- tables of the syntax ----
// full-bandwidth channels (A/52 table 5.8; 8, 9: one programme of 1+1, 10: Dolby); the mix levels; the bit-allocation band the
// coupling channel starts in; the first bin of a rematrixing band (4: the end of the last)
DSYN_FN int dsyn_nfchans(int acmod) { constexpr uint8_t k_nfchans[11] = {2, 1, 2, 3, 3, 4, 4, 5, 1, 1, 2}; return k_nfchans[acmod]; }
DSYN_FN float dsyn_clev(int c) { constexpr float k_clev[4] = {(float)AC3MI_G_3DB, (float)AC3MI_G_45DB, (float)AC3MI_G_6DB, (float)AC3MI_G_45DB}; return k_clev[c]; }
DSYN_FN float dsyn_slev(int c) { constexpr float k_slev[4] = {(float)AC3MI_G_3DB, (float)AC3MI_G_6DB, 0.f, (float)AC3MI_G_6DB}; return k_slev[c]; }
DSYN_FN int dsyn_cpl_bnd0(int begf) { constexpr uint8_t k_cpl_bnd0[16] = {31, 35, 37, 39, 41, 42, 43, 44, 45, 45, 46, 46, 47, 47, 48, 48}; return k_cpl_bnd0[begf]; }
DSYN_FN int dsyn_remat_edge(int band) { constexpr int k_remat_edge[5] = {13, 25, 37, 61, 253}; return k_remat_edge[band]; }

// a field of n flags (n codes of two bits), the first channel's in its top bits -> channel i's at bit i (2 i)
DSYN_FN uint32_t dsyn_rev(uint32_t v)
{
#if defined(__clang__)
    return __builtin_bitreverse32(v);
#else
    uint32_t r = 0;
    for (int i = 0; i < 32; i++) r |= ((v >> i) & 1u) << (31 - i);
    return r;
#endif
}
DSYN_FN int dsyn_flags(uint32_t field, int n) { return (int)(dsyn_rev(field) >> (32 - n)); }
DSYN_FN int dsyn_codes2(uint32_t field, int n)
{
    const uint32_t r = dsyn_rev(field) >> (32 - 2 * n);           // channel order right, each code's bits swapped
    return (int)(((r & 0x55555555u) << 1) | ((r >> 1) & 0x55555555u));
}

// The BSI behind lfeon, which the decoder reads past: dialnorm, compr, langcod, audprodi (twice for 1+1), copyrightb + origbs,
// the two timecodes, addbsi
template <class R>
DSYN_FN void dsyn_skip_bsi_tail(R &rd, bool dual_mono)
{
    int twice = dual_mono;
    do {
        rd.get(5);
        if (rd.get(1)) rd.get(8);
        if (rd.get(1)) rd.get(8);
        if (rd.get(1)) rd.get(7);
    } while (twice--);
    rd.get(2);
    if (rd.get(1)) rd.get(14);
    if (rd.get(1)) rd.get(14);
    if (rd.get(1)) {
        int len = rd.get(6);
        do rd.get(8); while (len--);
    }
}

// what a call expects of its frames and asks of a52_frame: the batch's lfeon, the requested output flags and level, whether
// dynamic-range words are applied (0 / 1)
struct DsynRequest {
    int lfeon, flags;
    float level;
    int dynrng_on;
};

// ---- a52_frame (parse.c:131-205) behind the sync-rule test: rd stands behind acmod (bit 51), acmod0 is the head's ----
// Returns the output liba52 grants (with A52_LFE), or -1: a frame the batch cannot hold (another lfeon) or a request it refuses
template <class R, class S>
DSYN_FN int dsyn_frame(R &rd, S &st, int acmod0, const DsynRequest &q)
{
    int acmod = acmod0;
    if (acmod == 2 && rd.get(2) == 2) acmod = 10;                 // dsurmod -> DOLBY
    float clev = 0.f, slev = 0.f;
    if ((acmod & 1) && acmod != 1) clev = dsyn_clev(rd.get(2));
    if (acmod & 4) slev = dsyn_slev(rd.get(2));
    st.set_clev(clev);
    st.set_slev(slev);
    const int lfeon = rd.get(1);
    st.set_lfeon(lfeon);
    if (lfeon != q.lfeon) return -1;
    float level = q.level;
    int output = a52_downmix_init_hd(acmod, q.flags, &level, clev, slev);
    if (output < 0) return -1;
    if (lfeon && (q.flags & 16)) output |= 16;                    // A52_LFE
    st.set_output(output);
    st.set_level(level * 2);
    st.set_dynrng(level * 2);
    st.set_dynrnge(q.dynrng_on);
    st.reset_deltbae();                                           // every slot's deltbae 2 (none) at each frame
    dsyn_skip_bsi_tail(rd, !acmod);
    st.set_nf(dsyn_nfchans(acmod0));
    return output;
}

// what a block's first half leaves for the kernel and for the second half
struct DsynBlock {
    int blkswm, dithmask;               // bit ch
    int reuse0;                         // block 0 takes exponents, coupling or bit-allocation parameters the frame did not send
    int cplexpstr, lfeexpstr, chexp;    // chexp: 2 bits per channel
    int redo;                           // slots that need a new bit allocation: bits 0..4 fbw, 5 lfe, 6 coupling channel
};

// ---- an audio block, first half: parse.c:572-736 ----
template <class R, class S, class K>
DSYN_FN int dsyn_block_a(R &rd, S &st, K &k, DsynBlock &b, int blk, int acmod, int nf, int lfeon)
{
    b = DsynBlock{0, 0, 0, 0, 0, 0, 0};
    b.blkswm = dsyn_flags(rd.get(nf), nf);                        // blksw[ch], dithflag[ch]
    b.dithmask = dsyn_flags(rd.get(nf), nf);
    int twice = !acmod, word = 0;
    do {                                                          // dynrnge, dynrng (dynrng2e, dynrng2)
        if (rd.get(1)) {
            const int code = rd.sget(8);
            const bool apply = st.dynrnge() != 0;
            const float range = k.dynrng(code, word, apply);
            if (apply) st.set_dynrng(st.level() * range);
        }
        word++;
    } while (twice--);
    k.lap(0);

    int chincpl = st.chincpl();
    if (rd.get(1)) {                                              // cplstre
        chincpl = 0;
        if (rd.get(1)) {                                          // cplinu
            chincpl = dsyn_flags(rd.get(nf), nf);
            st.set_chincpl(chincpl);
            if (acmod < 2) return 1;                      // (tests/dec_syntax_c tells the four exits apart by the last field read: here chincpl, nf bits)
            if (acmod == 2) st.set_phsflginu((int)rd.get(1));
            const int begf = rd.get(4), endf = rd.get(4);
            if (endf + 3 - begf < 0) return 1;            // (there: behind cplendf, 4 bits)
            const int nsub = endf + 3 - begf;
            st.set_cplstrtbnd(dsyn_cpl_bnd0(begf));
            st.set_cplstrtmant(begf * 12 + 37);
            st.set_endm(6, endf * 12 + 73);
            int ncplbnd = nsub;
            uint32_t strc = 0;
            for (int i = 0; i < nsub - 1; i++)
                if (rd.get(1)) { strc |= 1u << i; ncplbnd--; }
            st.set_cplbndstrc(strc);
            st.set_ncplbnd(ncplbnd);
        } else st.set_chincpl(0);
    } else if (blk == 0) b.reuse0 = 1;
    if (chincpl) {                                                // coupling coordinates
        const int ncplbnd = st.ncplbnd();
        int any = 0;
        for (int i = 0; i < nf; i++)
            if ((chincpl >> i) & 1) {
                if (rd.get(1)) {
                    const int master = 3 * (int)rd.get(2);
                    any = 1;
                    for (int j = 0; j < ncplbnd; j++) {
                        const int ex = rd.get(4), ma = rd.get(4);
                        k.cplco(i, j, ex, ma, master);
                    }
                } else if (blk == 0) b.reuse0 = 1;
            }
        if (acmod == 2 && st.phsflginu() && any)
            for (int j = 0; j < ncplbnd; j++)
                if (rd.get(1)) k.cplco_flip(j);
    }
    if (acmod == 2) {
        if (rd.get(1)) {                                          // rematstr
            const int end = chincpl ? st.cplstrtmant() : 253;
            int i = 0, flg = 0;
            do flg |= (int)rd.get(1) << i; while (dsyn_remat_edge(1 + i++) < end);
            st.set_rematflg(flg);
        } else if (blk == 0) b.reuse0 = 1;
    }
    k.lap(1);
    if (chincpl) b.cplexpstr = rd.get(2);
    b.chexp = dsyn_codes2(rd.get(2 * nf), nf);                    // chexpstr[ch]
    if (lfeon) b.lfeexpstr = rd.get(1);
    if (blk == 0) {
        if (chincpl && !b.cplexpstr) b.reuse0 = 1;
        if (lfeon && !b.lfeexpstr) b.reuse0 = 1;
        for (int i = 0; i < nf; i++) if (!((b.chexp >> (2 * i)) & 3)) b.reuse0 = 1;
    }
    const int cplstrtmant = st.cplstrtmant(), cplendmant = st.endm(6);
    for (int i = 0; i < 5; i++)
        if (i < nf && ((b.chexp >> (2 * i)) & 3)) {
            if ((chincpl >> i) & 1) st.set_endm(i, cplstrtmant);
            else {
                const int bw = rd.get(6);                         // chbwcod
                if (bw > 60) return 1;                    // (there: behind chbwcod, 6 bits)
                st.set_endm(i, bw * 3 + 73);
            }
        }
    k.lap(2);

    // exponent fields: parse.c:703-736
    if (b.cplexpstr) {
        const int ngrp = (cplendmant - cplstrtmant) / (3 << (b.cplexpstr - 1));
        const int e0 = (int)rd.get(4) << 1;
        b.redo = 64;
        if (k.exponents(6, b.cplexpstr, ngrp, e0, cplstrtmant, rd.pos())) return 1;
        rd.skip(7 * ngrp);
    }
    DSYN_UNROLL                                                   // (a constant slot: St's fields and the rows by constant shifts and offsets)
    for (int i = 0; i < 5; i++) {
        const int es = (b.chexp >> (2 * i)) & 3;
        if (i < nf && es) {
            const int gs = 3 << (es - 1), ngrp = (st.endm(i) + gs - 4) / gs;
            b.redo |= 1 << i;
            const int e0 = rd.get(4);
            if (k.exponents(i, es, ngrp, e0, 0, rd.pos())) return 1;
            rd.skip(7 * ngrp);
            rd.get(2);                                            // gainrng
        }
    }
    if (b.lfeexpstr) {
        b.redo |= 32;
        const int e0 = rd.get(4);
        if (k.exponents(5, b.lfeexpstr, 2, e0, 0, rd.pos())) return 1;
        rd.skip(14);
    }
    return 0;
}

// ---- second half: bit-allocation parameters and delta bit allocation, parse.c:738-772 ----
// b.redo comes in as the first half left it; b.reuse0 is added to
template <class R, class S, class K>
DSYN_FN int dsyn_block_b(R &rd, S &st, K &k, DsynBlock &b, int blk, int nf, int lfeon)
{
    const int chincpl = st.chincpl();
    if (rd.get(1)) { b.redo = 127; st.set_bai((int)rd.get(11)); }  // baie: sdcycod, fdcycod, sgaincod, dbpbcod, floorcod
    else if (blk == 0) b.reuse0 = 1;
    if (rd.get(1)) {                                              // snroffste
        b.redo = 127;
        st.set_csnroffst((int)rd.get(6));
        if (chincpl) st.set_cbai(6, (int)rd.get(7));
        for (int i = 0; i < 5; i++) if (i < nf) st.set_cbai(i, (int)rd.get(7));
        if (lfeon) st.set_cbai(5, (int)rd.get(7));
    } else if (blk == 0) b.reuse0 = 1;
    if (chincpl) {
        if (rd.get(1)) {                                          // cplleake
            b.redo |= 64;
            st.set_cplfleak(9 - (int)rd.get(3));
            st.set_cplsleak(9 - (int)rd.get(3));
        } else if (blk == 0) b.reuse0 = 1;
    }
    if (rd.get(1)) {                                              // deltbaie
        b.redo = 127;
        if (chincpl) st.set_deltbae(5, (int)rd.get(2));
        for (int i = 0; i < 5; i++) if (i < nf) st.set_deltbae(i, (int)rd.get(2));
        for (int pass = 0; pass < 6; pass++) {
            const int slot = pass == 0 ? 5 : pass - 1;            // cpl first, then fbw (parse.c:763-771)
            if (pass > nf) continue;
            if (slot == 5 && !chincpl) continue;
            if (st.deltbae(slot) != 1) continue;
            k.deltba_clear(slot);                                 // parse_deltba: parse.c:272-294
            int nseg = rd.get(3), band = 0;
            do {
                band += (int)rd.get(5);
                const int len = rd.get(4);
                int d = rd.get(3);
                d -= (d >= 4) ? 3 : 4;
                if (!len) continue;
                if (band + len >= 50) return 1;           // (there: behind a segment's delta, 3 bits)
                k.deltba_seg(slot, band, len, d);
                band += len;
            } while (nseg--);
        }
    }
    return 0;
}

// ---- the skip field: parse.c:800-804 ----
template <class R>
DSYN_FN void dsyn_skip_field(R &rd)
{
    if (rd.get(1)) {                                              // skiple
        const int n = rd.get(9);
        rd.skip(8 * n);
    }
}

}  // namespace ac3mi
