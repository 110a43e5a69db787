// thj_bamenc_fusion.h -- a fusion alignment as the two BAM records print_bamhit writes for it (bwt_map.cpp:1888-2093 with
// extract_partial_hits, :2148-2347; both records through GBamRecord, common.cpp:1005-1173): the ops before the fusion op on contig
// ref_id, the ops after it on contig ref_id2 = cigar[15], each with the read's name, the flag, MAPQ 255, the mate fields "*", 0, 0,
// its piece of the bases and qualities, the whole alignment's AS XM XO XG MD NM [XS], and then
//     XF:Z:<1|2> <name1>-<name2> <left + 1> <full cigar text> <SEQ> <QUAL + 33>
// Byte for byte what the host encoder (host/thj_bamrec.h, encode_aln's fusion branch) writes.  SEQ is the read in the alignment's
// orientation (reverse-complemented for THJ_HIT_ANTISENSE: anything but A C G T becomes N), cut at left_part_len = the ops 1..4
// before the fusion op; piece 1 is reverse-complemented again for RF / RR and its ops reversed, piece 2 for FR / RR.  A nibble that
// is never reversed stays what it was.
//   fusion_shape   serial: the sizes of both records (size2 == 0: a plain alignment, size1 is record_shape's), the read id, and
//                  whether the host encoder must take it;
//   fusion_write   a wave per alignment, on an execution context X (X::lane; GpuX in thj_bamout.hip, SimX in tests/xfsim): the
//                  name, the packed bases, the qualities and the two text copies inside XF:Z go a lane per output byte, the
//                  orientation resolved per lane from the raw nibbles; the CIGAR words go a lane each, the header words, the integer
//                  tags and the decimal text are lane 0's (a wave runs its lanes' different branches one after the other anyway).  No private arrays: every table is a packed constant.
// Contig names come as one byte blob with offsets: name of contig r (1-based) = names[name_off[r - 1] .. name_off[r]).
#pragma once
#include "thj_bamenc_core.h"

namespace bamenc {

constexpr uint64_t pack8(const char* s) {
    uint64_t v = 0;
    for (int i = 0; i < 8; ++i) v |= (uint64_t)(uint8_t)s[i] << (8 * i);
    return v;
}
// the letter of a base nibble (bam_nt16_rev_table)
THJ_DFN uint32_t nt16_letter(uint32_t nib) {
    constexpr uint64_t lo = pack8("=ACMGRSV"), hi = pack8("TWYHKDBN");
    return (uint32_t)(((nib & 8u) ? hi : lo) >> (8 * (nib & 7u))) & 0xFFu;
}
// the letter of a cigar op in XF:Z's cigar text (print_bamhit; ops without a letter print as the NUL they are there)
THJ_DFN uint32_t cigar_letter(uint32_t op) {
    constexpr uint64_t lo = pack8("\0MmIiDdF"), hi = pack8("FFFNnS\0\0");
    return (uint32_t)(((op & 8u) ? hi : lo) >> (8 * (op & 7u))) & 0xFFu;
}
// reverse_complement's complement (reads.cpp:189-207): anything but A C G T becomes N
THJ_DFN uint32_t comp_nib(uint32_t nib) { return nib == 1 ? 8u : nib == 2 ? 4u : nib == 4 ? 2u : nib == 8 ? 1u : 15u; }

THJ_DFN uint32_t dec_len(uint32_t v) {
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u : v < 100000000u ? 8u :
           v < 1000000000u ? 9u : 10u;
}
THJ_DFN uint8_t* put_dec(uint8_t* o, uint32_t v) {
    const uint32_t n = dec_len(v);
    for (uint32_t i = n; i-- > 0;) { o[i] = (uint8_t)('0' + v % 10u); v /= 10u; }
    return o + n;
}
THJ_DFN uint32_t sdec_len(int32_t v) { return v < 0 ? 1u + dec_len(0u - (uint32_t)v) : dec_len((uint32_t)v); }
THJ_DFN uint8_t* put_sdec(uint8_t* o, int32_t v) {
    if (v < 0) { *o++ = '-'; return put_dec(o, 0u - (uint32_t)v); }
    return put_dec(o, (uint32_t)v);
}

// what one pass over the cigar tells about a fusion alignment (encode_aln's loops)
struct FusionWalk {
    int32_t fi;                       // index of the (first) fusion op; < 0: a plain alignment
    uint32_t fdir;                    // THJ_CIG_FUSION_*
    int32_t rlen, indel, left_part;   // the read's length by the cigar, NM's indel share, the read bases before the fusion op
    int32_t fusion_left, fusion_right, right;
    uint32_t text_len;                // characters of the full cigar text
    bool spliced, second;             // a REF_SKIP op; a second fusion op
};
THJ_DFN FusionWalk fusion_walk(const thj_aln& a) {
    FusionWalk w;
    w.fi = -1; w.fdir = 0; w.rlen = 0; w.indel = 0; w.left_part = 0; w.fusion_left = -1; w.fusion_right = -1; w.right = a.left; w.text_len = 0;
    w.spliced = false; w.second = false;
    const int n = a.n_cigar < 16 ? a.n_cigar : 16;
#pragma unroll 1
    for (int k = 0; k < n; ++k) {
        const uint32_t c = a.cigar[k], op = c >> 28, len = c & 0x0FFFFFFFu;
        const bool fus = op >= THJ_CIG_FUSION_FF && op <= THJ_CIG_FUSION_RR;
        if (op == 1 || op == 2 || op == 3 || op == 4 || op == 13) w.rlen += (int32_t)len;
        if (op >= 3 && op <= 6) w.indel += (int32_t)len;
        if (op == 11 || op == 12) w.spliced = true;
        w.text_len += dec_len(fus ? len + 1u : len) + 1u;
        if (op == 1 || op == 11 || op == 5) w.right += (int32_t)len;
        else if (op == 2 || op == 12 || op == 6) w.right -= (int32_t)len;
        else if (fus) { w.fusion_left = (op == 7 || op == 8) ? w.right - 1 : w.right + 1; w.fusion_right = w.right = (int32_t)len; }
        if (fus) { if (w.fi < 0) { w.fi = k; w.fdir = op; } else w.second = true; }
        if (w.fi < 0 && op >= 1 && op <= 4) w.left_part += (int32_t)len;
    }
    return w;
}

// bytes of the tags both records share: AS XM XO XG MD NM [XS]
THJ_DFN uint32_t shared_tag_bytes(const thj_aln& a, int32_t indel, bool spliced) {
    return (3u + int_bytes((int)a.AS)) + (3u + int_bytes((int)a.XM)) + (3u + int_bytes((int)a.XO)) + (3u + int_bytes((int)a.XG)) + (4u + (uint32_t)a.md_len) +
           (3u + int_bytes((int)a.mismatches + indel)) + (spliced ? 4u : 0u);
}

struct FusionShape { uint32_t size1, size2; bool host_only; int64_t rid; };

// raw: the read's BAM record after its block_size field; n_ref: contigs of the run (name_off has n_ref + 1 entries)
THJ_DFN FusionShape fusion_shape(const thj_aln& a, const uint8_t* raw, const uint32_t* name_off, int32_t n_ref) {
    FusionShape f;
    const FusionWalk w = fusion_walk(a);
    if (w.fi < 0) {
        const Shape s = record_shape(a, raw);
        f.size1 = s.size; f.size2 = 0; f.host_only = s.host_only; f.rid = s.rid;
        return f;
    }
    const uint32_t l_rn = rd32(raw + 8) & 0xFFu, lseq = rd32(raw + 16), ref_id2 = a.cigar[15];
    f.size1 = 0; f.size2 = 0;
    f.rid = name_id(raw);
    f.host_only = a.n_cigar > 15 || w.second || a.md_len == THJ_MD_ON_HOST || (int32_t)lseq != w.rlen || l_rn == 0 || ref_id2 < 1 || ref_id2 > (uint32_t)n_ref;
    if (f.host_only) return f;
    const uint32_t len1 = (uint32_t)w.left_part < lseq ? (uint32_t)w.left_part : lseq, len2 = lseq - len1;
    const uint32_t n1 = (uint32_t)w.fi, n2 = (uint32_t)a.n_cigar - n1 - 1u;
    const uint32_t ln1 = name_off[a.ref_id] - name_off[a.ref_id - 1], ln2 = name_off[ref_id2] - name_off[ref_id2 - 1];
    // "XF" 'Z' <1|2> ' ' name1 '-' name2 ' ' left+1 ' ' cigar ' ' SEQ ' ' QUAL NUL
    const uint32_t xf = 3u + 2u + ln1 + 1u + ln2 + 1u + sdec_len(a.left + 1) + 1u + w.text_len + 1u + lseq + 1u + lseq + 1u;
    const uint32_t both = 36u + l_rn + shared_tag_bytes(a, w.indel, w.spliced) + xf;
    f.size1 = both + 4u * n1 + ((len1 + 1u) >> 1) + len1;
    f.size2 = both + 4u * n2 + ((len2 + 1u) >> 1) + len2;
    return f;
}

// Record 1 (part 0) or 2 (part 1) of the alignment at o; returns its size.  fusion_shape(a, ...) is not host_only and size2 != 0;
// tid_of_ref[ref_id - 1] = the contig's index in the output header.  Every lane of the wave calls it with the same arguments; x.lane = 0..63.
template <class X>
THJ_DFN uint32_t fusion_write_part(X& x, const thj_aln& a, const uint8_t* raw, const uint8_t* names, const uint32_t* name_off, const int32_t* tid_of_ref, uint32_t part,
                                   uint8_t* o) {
    const uint32_t lane = (uint32_t)x.lane;
    const FusionWalk w = fusion_walk(a);
    const uint32_t l_rn = rd32(raw + 8) & 0xFFu, lseq = rd32(raw + 16), ref_id2 = a.cigar[15];
    const uint32_t sq = 32u + l_rn + 4u * (rd32(raw + 12) & 0xFFFFu), ql = sq + ((lseq + 1u) >> 1);      // the read's bases and qualities, from raw
    const bool anti = (a.flags & THJ_HIT_ANTISENSE) != 0;
    const uint32_t lp = (uint32_t)w.left_part < lseq ? (uint32_t)w.left_part : lseq;
    {
        // the piece: its contig, where it starts, its ops (index c0, c0 + cs, ...) and its bases (index s0 + k, or s0 - k complemented,
        // of the read in the alignment's orientation)
        const bool rev = part ? (w.fdir == THJ_CIG_FUSION_FR || w.fdir == THJ_CIG_FUSION_RR) : (w.fdir == THJ_CIG_FUSION_RF || w.fdir == THJ_CIG_FUSION_RR);
        const uint32_t nc = part ? (uint32_t)a.n_cigar - (uint32_t)w.fi - 1u : (uint32_t)w.fi;
        const uint32_t len = part ? lseq - lp : lp;
        const int32_t c0 = part ? (rev ? (int32_t)a.n_cigar - 1 : w.fi + 1) : (rev ? w.fi - 1 : 0), cs = rev ? -1 : 1;
        const uint32_t s0 = part ? (rev ? lseq - 1u : lp) : (rev ? lp - 1u : 0u);
        // the fields in the record's order; `at` runs along.  Small fields go to lane 0, bulk fields a lane per output byte.
        if (lane == 0) {
            const uint32_t ref = part ? ref_id2 : a.ref_id;
            const int32_t left = part ? ((w.fdir == THJ_CIG_FUSION_FF || w.fdir == THJ_CIG_FUSION_RF) ? w.fusion_right : w.right + 1)
                                      : ((w.fdir == THJ_CIG_FUSION_FF || w.fdir == THJ_CIG_FUSION_FR) ? a.left : w.fusion_left);
            const int32_t pos = left + 1 <= 0 ? -1 : left;
            int32_t rend = pos;
            for (uint32_t i = 0; i < nc; ++i) { const uint32_t c = a.cigar[c0 + cs * (int32_t)i], op = bam_op(c >> 28); if (op == 0 || op == 2 || op == 3) rend += (int32_t)(c & 0x0FFFFFFFu); }
            const uint32_t bin = reg2bin(pos, nc == 0 ? pos + 1 : rend);
            wr32(o + 4, (uint32_t)tid_of_ref[ref - 1]); wr32(o + 8, (uint32_t)pos); wr32(o + 12, (bin << 16) | (255u << 8) | l_rn);
            wr32(o + 16, ((anti ? 0x10u : 0u) << 16) | nc); wr32(o + 20, len); wr32(o + 24, 0xFFFFFFFFu); wr32(o + 28, 0xFFFFFFFFu); wr32(o + 32, 0);
        }
        uint32_t at = 36u;
        for (uint32_t k = lane; k < l_rn; k += 64) o[at + k] = k + 1 < l_rn ? raw[32 + k] : (uint8_t)0;
        at += l_rn;
        if (lane < nc) {
            const uint32_t c = a.cigar[c0 + cs * (int32_t)lane];
            wr32(o + at + 4 * lane, ((c & 0x0FFFFFFFu) << 4) | bam_op(c >> 28));
        }
        at += 4u * nc;
        for (uint32_t b = lane; b < ((len + 1u) >> 1); b += 64) {
            uint32_t v = 0;
            for (uint32_t h = 0; h < 2; ++h) {
                const uint32_t k = 2 * b + h;
                if (k >= len) break;
                const uint32_t j = rev ? s0 - k : s0 + k;                  // in the alignment's orientation
                const uint32_t r = anti ? lseq - 1u - j : j;               // in the read's record
                uint32_t nib = (raw[sq + (r >> 1)] >> ((r & 1u) ? 0 : 4)) & 0xFu;
                if (anti) nib = comp_nib(nib);
                if (rev) nib = comp_nib(nib);
                v |= nib << (h ? 0 : 4);
            }
            o[at + b] = (uint8_t)v;
        }
        at += (len + 1u) >> 1;
        for (uint32_t k = lane; k < len; k += 64) {
            const uint32_t j = rev ? s0 - k : s0 + k;
            o[at + k] = raw[ql + (anti ? lseq - 1u - j : j)];
        }
        at += len;
        // AS XM XO XG MD NM [XS]
        const uint32_t at_md = at + (3u + int_bytes((int)a.AS)) + (3u + int_bytes((int)a.XM)) + (3u + int_bytes((int)a.XO)) + (3u + int_bytes((int)a.XG));
        const int nm = (int)a.mismatches + w.indel;
        if (lane == 0) {
            uint8_t* p = put_int(o + at, 'A', 'S', (int)a.AS);
            p = put_int(p, 'X', 'M', (int)a.XM); p = put_int(p, 'X', 'O', (int)a.XO); p = put_int(p, 'X', 'G', (int)a.XG);
            p[0] = 'M'; p[1] = 'D'; p[2] = 'Z'; p[3 + a.md_len] = 0;
            p = put_int(p + 4 + a.md_len, 'N', 'M', nm);
            if (w.spliced) { p[0] = 'X'; p[1] = 'S'; p[2] = 'A'; p[3] = (a.flags & THJ_HIT_ANTISENSE_SPLICE) ? '-' : '+'; }
        }
        for (uint32_t k = lane; k < a.md_len; k += 64) o[at_md + 3 + k] = (uint8_t)a.md[k];
        at = at_md + 4u + a.md_len + 3u + int_bytes(nm) + (w.spliced ? 4u : 0u);
        // "XFZ<1|2> " name1 '-' name2 ' ' left+1 ' ' cigar ' ' SEQ ' ' QUAL NUL
        if (lane == 0) { o[at] = 'X'; o[at + 1] = 'F'; o[at + 2] = 'Z'; o[at + 3] = part ? '2' : '1'; o[at + 4] = ' '; }
        at += 5u;
        {
            const uint32_t b1 = name_off[a.ref_id - 1], ln1 = name_off[a.ref_id] - b1;
            for (uint32_t k = lane; k < ln1; k += 64) o[at + k] = names[b1 + k];
            at += ln1;
            const uint32_t b2 = name_off[ref_id2 - 1], ln2 = name_off[ref_id2] - b2;
            for (uint32_t k = lane; k < ln2; k += 64) o[at + 1 + k] = names[b2 + k];
            if (lane == 0) { o[at] = '-'; o[at + 1 + ln2] = ' '; }
            at += ln2 + 2u;
        }
        const uint32_t at_seq = at + sdec_len(a.left + 1) + 1u + w.text_len + 1u;
        if (lane == 0) {
            uint8_t* p = put_sdec(o + at, a.left + 1);
            *p++ = ' ';
            for (int k = 0; k < a.n_cigar; ++k) {
                const uint32_t c = a.cigar[k], op = c >> 28, l = c & 0x0FFFFFFFu;
                p = put_dec(p, op >= THJ_CIG_FUSION_FF && op <= THJ_CIG_FUSION_RR ? l + 1u : l);
                *p++ = (uint8_t)cigar_letter(op);
            }
            *p = ' ';
            o[at_seq + lseq] = ' '; o[at_seq + 2u * lseq + 1u] = 0;
            wr32(o, at_seq + 2u * lseq + 2u - 4u);                         // block_size
        }
        for (uint32_t k = lane; k < lseq; k += 64) {
            const uint32_t r = anti ? lseq - 1u - k : k;
            const uint32_t nib = (raw[sq + (r >> 1)] >> ((r & 1u) ? 0 : 4)) & 0xFu;
            o[at_seq + k] = (uint8_t)nt16_letter(anti ? comp_nib(nib) : nib);
            o[at_seq + lseq + 1u + k] = (uint8_t)(raw[ql + r] + 33u);
        }
        return at_seq + 2u * lseq + 2u;
    }
}
// both records at o, back to back
template <class X>
THJ_DFN void fusion_write(X& x, const thj_aln& a, const uint8_t* raw, const uint8_t* names, const uint32_t* name_off, const int32_t* tid_of_ref, uint8_t* o) {
    // (one copy of the code, and -- as long as the caller does not promise that o aliases none of the inputs -- nothing carried from one
    // record to the other but o: hoisting everything the two records share out of this loop costs more scalar registers than there are)
#pragma unroll 1
    for (uint32_t part = 0; part < 2; ++part) o += fusion_write_part(x, a, raw, names, name_off, tid_of_ref, part, o);
}

}  // namespace bamenc
