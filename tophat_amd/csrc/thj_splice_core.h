// thj_splice_core.h -- SplicedBAMHitFactory::get_hit_from_buf + spliceCigar + getBAMmismatches (bwt_map.cpp:1469-1770, :681-883,
// :410-475) for one BAM record of a junction-db ("spliced") segment map: a segment mapped against a junction-db contig
// `name|left|l-r|right|type|strand` becomes a genomic hit with the REF_SKIP / DEL / INS operation spliced into its CIGAR.
// The same decisions, in the same order, as the host factory (host/thj_hostio.h: parse_spliced_hit), with the target's name
// tokenised once per run into a thj_juncdb_target instead of once per record.
// Plain per-record functions without memory of their own: thj_k_parse (thj_ingest.hip) calls them per thread, tests/splicesim
// compiles them for the CPU.  No private arrays: the input CIGAR is read from the record where it lies (the splice is one pass
// over it), the output CIGAR -- at most five operations -- lives in five named words.
// Fusion contigs (`fus` targets, strands ff / fr / rf / rr) are a compile-time choice: spliced_hit_as<true> splices them too -- the
// FUSION_xx operation at the break, the pieces that run down the genome in their lower-case forms, the second contig in the hit's
// last cigar word, at most four operations --, spliced_hit (= spliced_hit_as<false>) reports the record and the caller leaves the
// shard to the host factory.  tests/fusplicesim compiles spliced_hit_as<true> for the CPU.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/thj.h"

#ifndef THJ_DFN
#define THJ_DFN inline
#endif

namespace splc {

THJ_DFN uint32_t rd32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
THJ_DFN int popc64(uint64_t v) { return __builtin_popcountll(v); }

// what a record can report beside "kept" / "dropped" (bits of the status word)
enum { REP_CORRUPT = 1u, REP_CIGAR = 2u, REP_FUSION = 4u, REP_LONG_SEQ = 8u };

// qname "<id>|<offset>:<segment>:<segments>" (tophat.py:2948): insert_id = atoi, end = (segment + 1 == segments); q = the record's
// name, l_rn its length with the NUL
THJ_DFN void qname_id_end(const uint8_t* q, uint32_t l_rn, uint32_t& id, bool& end) {
    uint32_t v = 0, i = 0;
    while (i + 1 < l_rn && q[i] >= '0' && q[i] <= '9') { v = v * 10u + (uint32_t)(q[i] - '0'); ++i; }
    id = v;
    end = true;
    int pipe = -1;
    for (uint32_t k = 0; k + 1 < l_rn; ++k) if (q[k] == '|') pipe = (int)k;
    if (pipe < 0) return;
    bool colon = false;
    for (uint32_t k = (uint32_t)pipe + 1; k + 1 < l_rn; ++k) if (q[k] == ':') colon = true;
    if (!colon) return;
    // sscanf("%u:%u:%u"): a field without a digit ends the scan, the fields behind it stay 0 (bwt_map.cpp:1125-1143)
    uint32_t k = (uint32_t)pipe + 1, bb = 0, cc = 0;
    const uint32_t k0 = k;
    while (k + 1 < l_rn && q[k] >= '0' && q[k] <= '9') ++k;
    if (k > k0 && k + 1 < l_rn && q[k] == ':') {
        const uint32_t k1 = ++k;
        while (k + 1 < l_rn && q[k] >= '0' && q[k] <= '9') { bb = bb * 10u + (uint32_t)(q[k] - '0'); ++k; }
        if (k > k1 && k + 1 < l_rn && q[k] == ':') { ++k; while (k + 1 < l_rn && q[k] >= '0' && q[k] <= '9') { cc = cc * 10u + (uint32_t)(q[k] - '0'); ++k; } }
    }
    end = (bb + 1 == cc);
}

// the spliced CIGAR: up to five (op << 28 | length) words and the count of operations cigar_add appended (it may pass five:
// the sixth is the caller's loud outcome); `last` = the operation appended last, kept or not
struct Cig5 {
    uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, last = 0;
    int n = 0;
};
THJ_DFN void cig_set(Cig5& c, int k, uint32_t w) {
    switch (k) { case 0: c.c0 = w; break; case 1: c.c1 = w; break; case 2: c.c2 = w; break; case 3: c.c3 = w; break; case 4: c.c4 = w; break; default: break; }
}
THJ_DFN uint32_t cig_get(const Cig5& c, int k) {
    switch (k) { case 0: return c.c0; case 1: return c.c1; case 2: return c.c2; case 3: return c.c3; case 4: return c.c4; default: return 0; }
}
// cigar_add (bwt_map.cpp:672-678), quirk included: an op equal to the previous one extends it AND is appended again
THJ_DFN void cigar_add(Cig5& c, uint32_t op, int len) {
    if (len <= 0) return;
    if (c.n > 0 && (c.last >> 28) == op) {
        c.last = (op << 28) | (((c.last & 0x0FFFFFFFu) + (uint32_t)len) & 0x0FFFFFFFu);
        cig_set(c, c.n - 1, c.last);
    }
    c.last = (op << 28) | ((uint32_t)len & 0x0FFFFFFFu);
    cig_set(c, c.n, c.last);
    ++c.n;
}

// mismatch bits of the read offsets [a, b) (two words: a segment is at most 127 bases)
THJ_DFN int mm_in_range(uint64_t mm0, uint64_t mm1, int a, int b) {
    if (a < 0) a = 0;
    if (b > 128) b = 128;
    if (a >= b) return 0;
    const auto below = [](int k) -> uint64_t { return k <= 0 ? 0ull : k >= 64 ? ~0ull : ((1ull << k) - 1ull); };      // bits 0 .. k - 1
    const uint64_t m0 = below(b) & ~below(a), m1 = below(b - 64) & ~below(a - 64);
    return popc64(mm0 & m0) + popc64(mm1 & m1);
}

// BAM op ("MIDNSHP=X") -> CigarOpCode, 0 = the factory has no arm for it; H (5) is skipped by the callers
THJ_DFN uint32_t cig_code(uint32_t bop) { return bop == 0 ? 1u : bop == 1 ? 3u : bop == 2 ? 5u : bop == 3 ? 11u : bop == 4 ? 13u : bop == 6 ? 15u : 0u; }

// spliceCigar (bwt_map.cpp:681-865) for the codes INS (3), DEL (5) and REF_SKIP (11).  cg(i) = BAM cigar word i of the record (hard
// clips are passed over, as the factory never appends them); n_in = the operations it kept.  spl_mm is counted for INS only: for the
// other codes the reference computes a value nobody reads.  false: the factory drops the record.
template <class CG>
THJ_DFN bool splice_cigar(Cig5& out, CG cg, uint32_t n_cig, int n_in, uint64_t mm0, uint64_t mm1, int left, int spl_start, int spl_len, uint32_t spl_code, int& spl_mm) {
    const uint32_t INS = 3, DEL = 5, REF_SKIP = 11, MATCH = 1, PAD = 15, SOFT = 13;
    const int spl_ofs = spl_start - left;
    const int spl_ofs_end = spl_ofs + (spl_code == INS ? spl_len : 0);
    int ref_ofs = 0, read_ofs = 0;
    spl_mm = 0;
    // (spl_ofs_end <= 0, the alignment starting after the splice event, leaves the CIGAR as it is: the size test below drops it)
    if (spl_ofs_end <= 0) return false;
    for (uint32_t c = 0; c < n_cig; ++c) {
        const uint32_t w = cg(c);
        if ((w & 0xFu) == 5u) continue;
        const uint32_t op = cig_code(w & 0xFu);
        const int len = (int)(w >> 4);
        const int prev_read_ofs = read_ofs, cur_op_ofs = ref_ofs;
        if (op == MATCH) {
            ref_ofs += len; read_ofs += len;
            if (spl_code == INS) {
                const int lo = cur_op_ofs > spl_ofs ? cur_op_ofs : spl_ofs, hi = ref_ofs < spl_ofs_end ? ref_ofs : spl_ofs_end;
                spl_mm += mm_in_range(mm0, mm1, prev_read_ofs + (lo - cur_op_ofs), prev_read_ofs + (hi - cur_op_ofs));
            }
        } else if (op == DEL || op == REF_SKIP || op == PAD) ref_ofs += len;
        else if (op == SOFT || op == INS) read_ofs += len;
        if (cur_op_ofs >= spl_ofs_end || ref_ofs <= spl_ofs) {
            if (cur_op_ofs == spl_ofs_end && spl_code != INS && op != INS) cigar_add(out, spl_code, spl_len);
            cigar_add(out, op, len);
        } else if (spl_code == INS) {
            if (spl_ofs > cur_op_ofs) cigar_add(out, op, spl_ofs - cur_op_ofs);
            // (the reference's arm for an alignment that starts inside the inserted bases; no caller reaches it: get_hit_from_buf drops
            // left > lsp first, and then spl_ofs = lsp + 1 - left >= 1.  Restated for the sake of reading the two side by side)
            if (spl_ofs < 0) cigar_add(out, spl_code, spl_len + spl_ofs);
            else cigar_add(out, spl_code, spl_len);
            if (ref_ofs > spl_ofs_end) cigar_add(out, op, ref_ofs - spl_ofs_end);
        } else {
            cigar_add(out, op, spl_ofs - cur_op_ofs);
            cigar_add(out, spl_code, spl_len);
            cigar_add(out, op, ref_ofs - spl_ofs);
        }
    }
    if (out.n < n_in + 2) return false;
    if ((out.c0 >> 28) != MATCH || (out.last >> 28) != MATCH) return false;
    return true;
}

// spliceCigar for the fusion codes FUSION_FF .. FUSION_RR (7 .. 10; bwt_map.cpp:753-790, :822-853): spl_ofs is a distance, whichever
// way the first piece runs; the operations before an rf / rr break and after an fr / rr break come out lower-case (MATCH -> mATCH,
// INS -> iNS, DEL -> dEL, REF_SKIP -> rEF_SKIP: op + 1), "after" beginning where the fusion operation goes in -- the two halves of
// the operation that is split take one rule each.  spl_mm is left out: nobody reads it for these codes.
template <class CG>
THJ_DFN bool splice_cigar_fusion(Cig5& out, CG cg, uint32_t n_cig, int n_in, int left, int spl_start, int spl_len, uint32_t spl_code) {
    const uint32_t INS = 3, DEL = 5, REF_SKIP = 11, MATCH = 1, mATCH = 2, PAD = 15;
    const bool low_before = spl_code == 9u || spl_code == 10u, low_after = spl_code == 8u || spl_code == 10u;
    const auto lower = [](uint32_t op) { return (op == 1u || op == 3u || op == 5u || op == 11u) ? op + 1u : op; };
    const int spl_ofs = spl_start > left ? spl_start - left : left - spl_start;
    int ref_ofs = 0;
    bool xfound = false;
    if (spl_ofs <= 0) return false;
    for (uint32_t c = 0; c < n_cig; ++c) {
        const uint32_t w = cg(c);
        if ((w & 0xFu) == 5u) continue;
        const uint32_t op = cig_code(w & 0xFu);
        const int len = (int)(w >> 4);
        const int cur_op_ofs = ref_ofs;
        if (op == MATCH || op == DEL || op == REF_SKIP || op == PAD) ref_ofs += len;
        if (cur_op_ofs >= spl_ofs || ref_ofs <= spl_ofs) {
            if (cur_op_ofs == spl_ofs && op != INS) { xfound = true; cigar_add(out, spl_code, spl_len); }
            cigar_add(out, (xfound ? low_after : low_before) ? lower(op) : op, len);
        } else {
            xfound = true;
            cigar_add(out, low_before ? lower(op) : op, spl_ofs - cur_op_ofs);
            cigar_add(out, spl_code, spl_len);
            cigar_add(out, low_after ? lower(op) : op, ref_ofs - spl_ofs);
        }
    }
    if (out.n < n_in + 2) return false;
    const uint32_t first = out.c0 >> 28, last = out.last >> 28;
    if ((first != MATCH && first != mATCH) || (last != MATCH && last != mATCH)) return false;
    return true;
}

// getBAMmismatches: the mismatch positions of an MD string (NUL-terminated, at most n bytes) as bits over the read offset, and
// their number; positions at or past l_seq are counted and not marked
THJ_DFN int md_mismatches(const uint8_t* s, uint32_t n, uint32_t l_seq, uint64_t& mm0, uint64_t& mm1) {
    const auto digit = [](uint8_t ch) { return ch >= '0' && ch <= '9'; };
    const auto alpha = [](uint8_t ch) { return (ch >= 'A' && ch <= 'Z') || (ch >= 'a' && ch <= 'z'); };
    int num_mm = 0;
    uint32_t k = 0, bi = 0;
    mm0 = mm1 = 0;
    while (k < n && s[k]) {
        if (digit(s[k])) { uint32_t v = 0; while (k < n && digit(s[k])) { v = v * 10u + (uint32_t)(s[k] - '0'); ++k; } bi += v; }
        while (k < n && alpha(s[k])) {
            ++k; ++num_mm;
            if (bi < l_seq) { if (bi < 64u) mm0 |= 1ull << bi; else if (bi < 128u) mm1 |= 1ull << (bi - 64u); }
            ++bi;
        }
        if (k < n && s[k] == '^') { ++k; while (k < n && alpha(s[k])) { ++k; ++bi; } }
        if (k < n && s[k] && !digit(s[k]) && !alpha(s[k]) && s[k] != '^') ++k;
    }
    return num_mm;
}

// the hit of one record (as thj_span_hit's words: meta = flags | mismatches << 8 | edit_dist << 16 | n_cigar << 24)
struct Hit { uint32_t ref_id; int32_t left; uint32_t meta; uint32_t cigar[5]; };

// get_hit_from_buf for record `d` (after its block_size field, `bs` bytes) of a junction-db map whose targets are `tg`.  true: the
// factory keeps the record.  rep |= REP_*: REP_CORRUPT a header or tag that does not fit the record, REP_CIGAR a sixth spliced operation
// (the host factory stops the run there), REP_FUSION a record on a fusion contig, REP_LONG_SEQ more bases than the bitmap holds.
// FUSED: fusion contigs are spliced as well (bwt_map.cpp:1664-1759); REP_FUSION is never raised, REP_CIGAR is a fused hit's fifth
// operation -- its last cigar word holds the second contig.
template <bool FUSED>
THJ_DFN bool spliced_hit_as(const uint8_t* d, uint32_t bs, const thj_juncdb_target* tg, int64_t n_tg, int max_report_intron, uint32_t& id, Hit& h, uint32_t& rep) {
    const int32_t tid = (int32_t)rd32(d), pos = (int32_t)rd32(d + 4), mtid = (int32_t)rd32(d + 20);
    const uint32_t bin_mq_nl = rd32(d + 8), flag_nc = rd32(d + 12), l_seq = rd32(d + 16);
    const uint32_t l_rn = bin_mq_nl & 0xFF, n_cig = flag_nc & 0xFFFF, flag = flag_nc >> 16;
    id = 0;
    if (bs < 32u || l_rn == 0u || l_seq > 0x7FFFFFFFu || 32ull + l_rn + 4ull * n_cig + ((unsigned long long)l_seq + 1ull) / 2ull + l_seq > (unsigned long long)bs) { rep |= REP_CORRUPT; return false; }
    bool end;
    qname_id_end(d + 32, l_rn, id, end);
    if (tid < 0 || (flag & 4u)) return false;
    const uint8_t* cig = d + 32 + l_rn;
    int n_in = 0;
    for (uint32_t c = 0; c < n_cig; ++c) {
        const uint32_t w = rd32(cig + 4 * c), bop = w & 0xFu;
        if ((w >> 4) == 0) return false;
        if (bop == 5u) continue;
        if (cig_code(bop) == 0) return false;                    // '=' and 'X' too: the factory's switch has no arm for them
        if (bop == 3u && (int)(w >> 4) > max_report_intron) return false;
        ++n_in;
    }
    if (mtid >= 0 && mtid != tid) return false;
    // the first MD tag of the record (bam_aux_get), of type Z or H (bam_aux2Z takes both)
    uint64_t mm0 = 0, mm1 = 0;
    int num_mm = 0;
    uint32_t pp = 32 + l_rn + 4 * n_cig + (l_seq + 1) / 2 + l_seq;
    while (pp + 3 <= bs) {
        const char t0 = (char)d[pp], t1 = (char)d[pp + 1], ty = (char)d[pp + 2];
        pp += 3;
        const uint32_t fixed = (ty == 'A' || ty == 'c' || ty == 'C') ? 1u : (ty == 's' || ty == 'S') ? 2u : (ty == 'i' || ty == 'I' || ty == 'f') ? 4u : ty == 'd' ? 8u : ty == 'B' ? 5u : 0u;
        if (fixed > bs - pp) { rep |= REP_CORRUPT; return false; }
        if (ty == 'Z' || ty == 'H') {
            if (t0 == 'M' && t1 == 'D') {
                if (l_seq > 128u) { rep |= REP_LONG_SEQ; return false; }
                num_mm = md_mismatches(d + pp, bs - pp, l_seq, mm0, mm1);
                break;
            }
            while (pp < bs && d[pp]) ++pp;
            ++pp;
        } else if (ty == 'B') {
            const char st = (char)d[pp];
            const uint32_t cnt = rd32(d + pp + 1), sz = (st == 'c' || st == 'C') ? 1u : (st == 's' || st == 'S') ? 2u : 4u;
            if ((unsigned long long)cnt * sz > (unsigned long long)(bs - pp - 5u)) { rep |= REP_CORRUPT; return false; }
            pp += 5 + cnt * sz;
        } else if (fixed) pp += fixed;
        else pp = bs;
    }
    if (tid >= n_tg) return false;                               // (a target the header does not list)
    const thj_juncdb_target t = tg[tid];
    if (t.type == THJ_JUNCDB_INVALID) return false;
    // (reported for every record that got this far, also one the factory would go on to drop or whose id lies outside the caller's
    // shard, as REP_LONG_SEQ is: the shard then goes to the host factory, which is never wrong)
    if (!FUSED && t.type == THJ_JUNCDB_FUS) { rep |= REP_FUSION; return false; }
    const bool fused = FUSED && t.type == THJ_JUNCDB_FUS;
    int left = t.left + pos, lsp = t.lsp, spl_mm = 0;
    const auto cg = [cig](uint32_t c) { return rd32(cig + 4 * c); };
    Cig5 out;
    bool flipped = false;
    if (fused) {
        // on rf / rr contigs the first piece runs down the genome from the contig's left edge; a strand word that is none of the
        // four is FUSION_RR to the factory's if-chain, and flips nothing (juncs_db writes none such; with the four, a fused hit never
        // has THJ_HIT_ANTISENSE_SPLICE)
        flipped = t.strand == THJ_JUNCDB_RF || t.strand == THJ_JUNCDB_RR;
        if (flipped) left = t.left - pos;
        const uint32_t code = t.strand == THJ_JUNCDB_FF ? 7u : t.strand == THJ_JUNCDB_FR ? 8u : t.strand == THJ_JUNCDB_RF ? 9u : 10u;
        if (code >= 9u) { lsp -= 1; if (left <= lsp) return false; }
        else { lsp += 1; if (left >= lsp) return false; }
        if (!splice_cigar_fusion(out, cg, n_cig, n_in, left, lsp, t.second, code)) return false;
        if (t.ref_id2 == 0) return false;                        // a second contig the run does not know
    } else if (t.type == THJ_JUNCDB_INS) {
        if (left > lsp) return false;
        if (!splice_cigar(out, cg, n_cig, n_in, mm0, mm1, left, lsp + 1, t.second, 3u, spl_mm)) return false;
        num_mm -= spl_mm;
    } else {
        const int gap_len = t.second - lsp - 1;
        lsp += 1;
        if (left >= lsp) return false;
        if (!splice_cigar(out, cg, n_cig, n_in, mm0, mm1, left, lsp, gap_len, t.type == THJ_JUNCDB_DEL ? 5u : 11u, spl_mm)) return false;
    }
    if (out.n > (fused ? 4 : 5)) { rep |= REP_CIGAR; return false; }
    if (t.ref_id == 0) return false;                             // a contig the run does not know
    int gap = 0;
    for (int k = 0; k < 5; ++k) {
        const uint32_t w = k < out.n ? cig_get(out, k) : 0u, op = w >> 28;
        if (op >= 3u && op <= 6u) gap += (int)(w & 0x0FFFFFFFu);
        h.cigar[k] = w;
    }
    if (fused) h.cigar[4] = t.ref_id2;
    const uint32_t mm8 = (uint32_t)(uint8_t)num_mm, ed = (uint32_t)(uint8_t)(num_mm + gap);
    const uint32_t fl = ((((flag & 0x10u) != 0u) != flipped) ? THJ_HIT_ANTISENSE : 0u) | (end ? THJ_HIT_END : 0u) | (t.strand == THJ_JUNCDB_REV ? THJ_HIT_ANTISENSE_SPLICE : 0u) |
                        (flipped ? THJ_HIT_STRAND_FLIPPED : 0u) | (fused ? THJ_HIT_FUSED : 0u);
    h.ref_id = t.ref_id; h.left = left;
    h.meta = fl | (mm8 << 8) | (ed << 16) | ((uint32_t)out.n << 24);
    return true;
}
THJ_DFN bool spliced_hit(const uint8_t* d, uint32_t bs, const thj_juncdb_target* tg, int64_t n_tg, int max_report_intron, uint32_t& id, Hit& h, uint32_t& rep) {
    return spliced_hit_as<false>(d, bs, tg, n_tg, max_report_intron, id, h, rep);
}

}  // namespace splc
