// thj_accepted_core.h -- one reported alignment rewritten as tophat_reports writes it into accepted_hits.bam:
//
//   print_sam_for_single (index_vector, the primary draw)     tophat_reports.cpp:985-1025, lex_hit_sort :962-983
//   rewrite_sam_record, the unpaired overload (FRAG_UNPAIRED; FRAG_LEFT / FRAG_RIGHT for a side that goes alone)    tophat_reports.cpp:656-781
//   print_sam_for_pair, rewrite_sam_record's paired overload   tophat_reports.cpp:1027-1089, :783-960 (what differs: struct Mate)
//   add_auxData                                                tophat_reports.cpp:580-654
//   the text the reference goes through: bam_format1_core      bam.c:243-324
//   ... and back: GBamRecord (set_cigar, add_sequence, add_quals, add_aux)   common.cpp:1000-1194
//
// The reference formats the input record as a SAM line, edits the line's tokens and parses it into a new record.  Here the record
// is rewritten bytes to bytes; what the text round trip changes is restated field by field in emit().  One function makes every
// decision: emit() walks the input record once and hands what it writes to a sink.  With a sink that only counts it gives the
// output size and the loud flags (a lane per record); with a sink whose copies are spread over a wave it writes the record (a wave
// per record: every lane runs the same walk, so the walk's branches are uniform); with a sink over plain memory tests/acceptedsim
// runs it on the CPU.
//
// Not here: fusion alignments (XF:Z, two records: extract_partial_hits), XP:Z (fusion_search), --report-secondary-alignments.
#pragma once
#include <stdint.h>

#ifndef THJ_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define THJ_HD __host__ __device__ __forceinline__
#else
#define THJ_HD inline
#endif
#endif

namespace acc {

// what ends the run, with a message that names the case; never another answer
enum { LOUD_FUSION = 1u,        // a tag named XF: a fusion alignment (two records; not built)
       LOUD_TAGTYPE = 2u,       // a tag of type f, d, H or B (or of no BAM type)
       LOUD_Z = 4u,             // an empty Z value, or one holding a TAB: the reference's line of tokens cannot carry it
       LOUD_LSEQ0 = 8u,         // l_seq == 0
       LOUD_BIG = 16u,          // the rewritten record, its block_size field included, is over 64 KiB
       LOUD_PAIRED = 32u,       // mtid >= 0 or flag 0x1 in the INPUT: the sides of an insert come as single-end records
       LOUD_MALFORMED = 64u,    // the header, the cigar or a tag does not fit the record; a cigar op above 8
       LOUD_QLEN = 128u,        // the cigar's query length is not l_seq (add_sequence ends the reference's run)
       LOUD_CONTIG = 256u,      // the contig has no @SQ line in the output header
       LOUD_ORDER = 512u };     // (the pass, not the record) the replayed pieces do not line up with what was added

enum { LIB_FR_FIRSTSTRAND = 2, LIB_FR_SECONDSTRAND = 3 };      // thj_params.library_type's numbers; every other value: no XS:A is made
enum { SLOT_PRIMARY = 1u, SLOT_HAS_NEXT = 2u };

// rg[0 .. rg_len): --rg-id (rg_len 0: none); tid_of_ref[ref_id - 1] = the contig's index in the output header (< 0: none);
// names[name_off[r] .. name_off[r + 1]) = the name of contig r + 1; mapq[min(n, 5)] = MAPQ of a read with n reported alignments
struct Cfg { int32_t library_type; uint32_t rg_len; const uint8_t* rg; const int32_t* tid_of_ref; int32_t n_ref; const uint8_t* names; const uint32_t* name_off; uint8_t mapq[8]; };

// what a record's read gives it: n = hits.size(), place = its place in index_vector, the next record in index_vector order, the
// second pass's AlignStatus score, the alignment's contig; out = where the record goes among the piece's output records
struct Slot { uint32_t n, place, flags, ref_id, next_ref; int32_t next_left, score; uint32_t out; };

// What a record's insert gives it.  side: which read of the insert the record is (FRAG_UNPAIRED / FRAG_LEFT / FRAG_RIGHT: by the file it came
// from).  partner: the record is written with its mate (print_sam_for_pair): the mate's contig, left(), right(), antisense_align(), and
// happy() of the insert's best grade.  A side without a partner is one that --report-mixed-alignments sends down the single-end way.
// The default is the single-end writer's record.
enum { SIDE_UNPAIRED = 0, SIDE_LEFT = 1, SIDE_RIGHT = 2 };
struct Mate { uint32_t side = SIDE_UNPAIRED, partner = 0, ref_id = 0; int32_t left = 0, right = 0; uint32_t anti = 0, happy = 0; };

// TLEN of a record [left, right) whose partner [p_left, p_right) lies on the same contig (tophat_reports.cpp:864-875), as written there
THJ_HD int32_t tlen_of(int32_t left, int32_t right, int32_t p_left, int32_t p_right) {
    if (left <= p_left && right >= p_right && right - left > p_right - p_left) return right - left;              // it contains its partner
    if (p_left <= left && p_right >= right && p_right - p_left > right - left) return p_left - p_right;          // its partner contains it
    return left < p_left ? p_right - left : p_left - right;
}
// the FLAG bits the insert adds (:717-729 unpaired overload, :805-814 and :881-884 paired overload); 0x100 is the caller's
THJ_HD uint32_t mate_flag_bits(const Mate& m) {
    if (m.side == SIDE_UNPAIRED) return 0u;
    const uint32_t side = m.side == SIDE_LEFT ? 0x40u : 0x80u;
    if (!m.partner) return 0x1u | side | 0x8u;
    return 0x1u | side | (m.happy ? 0x2u : 0u) | (m.anti ? 0x20u : 0u);
}
// add_auxData's XS:A (:615-647): FRAG_RIGHT takes the other sign
THJ_HD char xs_strand(int32_t library_type, bool anti, uint32_t side) {
    const bool plus = ((library_type == LIB_FR_FIRSTSTRAND) == anti) != (side == SIDE_RIGHT);
    return plus ? '+' : '-';
}

THJ_HD uint32_t rd16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
THJ_HD uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// bam_reg2bin (bam.h:657-666) on the reference's own unsigned arithmetic
THJ_HD uint32_t reg2bin(uint32_t beg, uint32_t end) {
    --end;
    if (beg >> 14 == end >> 14) return 4681u + (beg >> 14);
    if (beg >> 17 == end >> 17) return 585u + (beg >> 17);
    if (beg >> 20 == end >> 20) return 73u + (beg >> 20);
    if (beg >> 23 == end >> 23) return 9u + (beg >> 23);
    if (beg >> 26 == end >> 26) return 1u + (beg >> 26);
    return 0u;
}

// add_aux's integer (common.cpp:1130-1171): the smallest type under ITS bounds -- c down to -127, s down to -32767
THJ_HD void int_type(int64_t x, char& ty, uint32_t& len) {
    if (x < 0) { if (x >= -127) { ty = 'c'; len = 1; } else if (x >= -32767) { ty = 's'; len = 2; } else { ty = 'i'; len = 4; } }
    else { if (x <= 255) { ty = 'C'; len = 1; } else if (x <= 65535) { ty = 'S'; len = 2; } else { ty = 'I'; len = 4; } }
}

// lex_hit_sort over (contig, left); records that tie stand in `hits` order (h = the place in hits, or anything that rises with it):
// what libstdc++'s std::sort gives for at most 16 entries, where it is an insertion sort
THJ_HD bool lex_before(uint32_t ref_a, int32_t left_a, uint32_t h_a, uint32_t ref_b, int32_t left_b, uint32_t h_b) {
    if (ref_a != ref_b) return ref_a < ref_b;
    if (left_a != left_b) return left_a < left_b;
    return h_a < h_b;
}
static constexpr uint32_t SORT_BY_COUNTING = 16;      // _S_threshold of libstdc++'s std::sort

// does v[0 .. n) hold the five bytes of `what`?
THJ_HD bool holds(const uint8_t* v, uint32_t n, const char* what) {
    for (uint32_t i = 0; i + 5u <= n; ++i)
        if (v[i] == (uint8_t)what[0] && v[i + 1] == (uint8_t)what[1] && v[i + 2] == (uint8_t)what[2] && v[i + 3] == (uint8_t)what[3] && v[i + 4] == (uint8_t)what[4]) return true;
    return false;
}

// a sink that only counts
struct NullSink {
    THJ_HD void copy(uint32_t, const uint8_t*, uint32_t) {}
    THJ_HD void fill(uint32_t, uint8_t, uint32_t) {}
    THJ_HD void put(uint32_t, uint32_t, uint32_t) {}
    THJ_HD void cigar(uint32_t, const uint8_t*, uint32_t) {}
};
// = and X become M (set_cigar, common.cpp:1060)
THJ_HD uint32_t cigar_word(uint32_t c) { const uint32_t op = c & 15u; return (op == 7u || op == 8u) ? (c & ~15u) : c; }
// plain memory
struct MemSink {
    uint8_t* o;
    THJ_HD void copy(uint32_t at, const uint8_t* src, uint32_t len) { for (uint32_t k = 0; k < len; ++k) o[at + k] = src[k]; }
    THJ_HD void fill(uint32_t at, uint8_t v, uint32_t len) { for (uint32_t k = 0; k < len; ++k) o[at + k] = v; }
    THJ_HD void put(uint32_t at, uint32_t v, uint32_t nbytes) { for (uint32_t k = 0; k < nbytes; ++k) o[at + k] = (uint8_t)(v >> (8u * k)); }
    THJ_HD void cigar(uint32_t at, const uint8_t* src, uint32_t n) { for (uint32_t k = 0; k < n; ++k) put(at + 4u * k, cigar_word(rd32(src + 4u * k)), 4u); }
};

template <class Sink>
THJ_HD uint32_t put_int_tag(Sink& out, uint32_t o, char k0, char k1, int64_t x) {
    char ty; uint32_t len;
    int_type(x, ty, len);
    out.put(o, (uint32_t)(uint8_t)k0 | ((uint32_t)(uint8_t)k1 << 8) | ((uint32_t)(uint8_t)ty << 16), 3u);
    out.put(o + 3u, (uint32_t)x, len);
    return o + 3u + len;
}

// Input record d (behind its block_size field, bs bytes) -> the rewritten record, block_size field first, through `out`.  Returns
// its size; loud collects LOUD_* (the size then means nothing).
template <class Sink>
THJ_HD uint32_t emit(const uint8_t* d, uint32_t bs, const Cfg& cfg, const Slot& s, Sink& out, uint32_t& loud, const Mate& m = Mate()) {
    if (bs < 32u) { loud |= LOUD_MALFORMED; return 0; }
    const uint32_t l_rn = d[8], flag_nc = rd32(d + 12), n_cig = flag_nc & 0xFFFFu, flag = flag_nc >> 16, pos = rd32(d + 4);
    const int32_t l_seq = (int32_t)rd32(d + 16), mtid = (int32_t)rd32(d + 20);
    if (l_seq < 0 || l_rn == 0u || 32ull + l_rn + 4ull * n_cig + ((uint64_t)l_seq + 1ull) / 2ull + (uint64_t)l_seq > (uint64_t)bs) { loud |= LOUD_MALFORMED; return 0; }
    if (mtid >= 0 || (flag & 1u)) loud |= LOUD_PAIRED;
    if (l_seq == 0) loud |= LOUD_LSEQ0;
    // QNAME: a C string; cut at its last '/' when fewer than 4 characters remain from there on (:711-714)
    uint32_t nl = 0, slash = 0xFFFFFFFFu;
    while (nl + 1u < l_rn && d[32u + nl]) { if (d[32u + nl] == '/') slash = nl; ++nl; }
    if (slash != 0xFFFFFFFFu && nl - slash < 4u) nl = slash;
    // the cigar as set_cigar reads it back: the end for the bin (bam_calend: M, D, N), the query length add_sequence checks (M, I, S)
    const uint8_t* cg = d + 32u + l_rn;
    uint32_t end = pos, qlen = 0;
    for (uint32_t k = 0; k < n_cig; ++k) {
        const uint32_t c = rd32(cg + 4u * k), op = c & 15u, len = c >> 4;
        if (op > 8u) loud |= LOUD_MALFORMED;
        if (op == 0u || op == 7u || op == 8u) { end += len; qlen += len; }
        else if (op == 2u || op == 3u) end += len;
        else if (op == 1u || op == 4u) qlen += len;
    }
    if (n_cig && qlen != (uint32_t)l_seq) loud |= LOUD_QLEN;
    const uint32_t bin = reg2bin(pos, n_cig ? end : pos + 1u) & 0xFFFFu;
    int32_t tid = -1;
    if (s.ref_id >= 1u && s.ref_id <= (uint32_t)cfg.n_ref) tid = cfg.tid_of_ref[s.ref_id - 1u];
    if (tid < 0) loud |= LOUD_CONTIG;
    const uint32_t n5 = s.n < 5u ? s.n : 5u;
    uint32_t o = 4;
    out.put(o, (uint32_t)tid, 4u); out.put(o + 4u, pos, 4u);
    out.put(o + 8u, (bin << 16) | ((uint32_t)cfg.mapq[n5] << 8) | (nl + 1u), 4u);
    out.put(o + 12u, (((flag | mate_flag_bits(m) | ((s.flags & SLOT_PRIMARY) ? 0u : 0x100u)) & 0xFFFFu) << 16) | n_cig, 4u);
    out.put(o + 16u, (uint32_t)l_seq, 4u);
    if (m.partner) {
        // "=" is the record's own target; another contig's is looked up by name (none: -1, and the partner's own record is loud)
        const bool same = m.ref_id == s.ref_id;
        int32_t mtid_out = tid;
        if (!same) mtid_out = (m.ref_id >= 1u && m.ref_id <= (uint32_t)cfg.n_ref) ? cfg.tid_of_ref[m.ref_id - 1u] : -1;
        if (mtid_out < 0) mtid_out = -1;
        out.put(o + 20u, (uint32_t)mtid_out, 4u);
        out.put(o + 24u, (uint32_t)m.left, 4u);
        out.put(o + 28u, same ? (uint32_t)tlen_of((int32_t)pos, (int32_t)end, m.left, m.right) : 0u, 4u);
    } else {
        out.put(o + 20u, 0xFFFFFFFFu, 4u);                       // mate "*"
        out.put(o + 24u, rd32(d + 24), 4u); out.put(o + 28u, rd32(d + 28), 4u);
    }
    o += 32u;
    out.copy(o, d + 32u, nl); out.put(o + nl, 0u, 1u); o += nl + 1u;
    out.cigar(o, cg, n_cig); o += 4u * n_cig;
    // SEQ: letters and back; the spare nibble of an odd length comes out 0 (add_sequence's memset)
    const uint8_t* sq = cg + 4u * n_cig;
    const uint32_t sb = ((uint32_t)l_seq + 1u) / 2u;
    if ((uint32_t)l_seq & 1u) { out.copy(o, sq, sb - 1u); out.put(o + sb - 1u, sq[sb - 1u] & 0xF0u, 1u); }
    else out.copy(o, sq, sb);
    o += sb;
    // QUAL: "*" when its first byte is 0xff (bam.c:286), which add_quals turns into 0xff throughout
    const uint8_t* ql = sq + sb;
    // (and a single base of quality 9 is the text "*" as well: add_quals reads it as no qualities)
    if (l_seq > 0 && (ql[0] == 0xFFu || (l_seq == 1 && ql[0] == 9u))) out.fill(o, 0xFFu, (uint32_t)l_seq); else out.copy(o, ql, (uint32_t)l_seq);
    o += (uint32_t)l_seq;
    // the tags, in the input's order.  A tag that comes out byte for byte as it went in joins the run of such tags before it, and a
    // run is moved as one span.
    uint32_t p = (uint32_t)(ql - d) + (uint32_t)l_seq, run_at = 0, run_len = 0;
    bool xs_found = false;
    while (p < bs) {
        if (p + 3u > bs) { loud |= LOUD_MALFORMED; break; }
        const char k0 = (char)d[p], k1 = (char)d[p + 1], ty = (char)d[p + 2];
        const uint32_t p0 = p;
        p += 3u;
        if (k0 == 'X' && k1 == 'F') loud |= LOUD_FUSION;          // strncmp(tok, "XF", 2), :681
        const uint32_t fixed = (ty == 'A' || ty == 'c' || ty == 'C') ? 1u : (ty == 's' || ty == 'S') ? 2u : (ty == 'i' || ty == 'I') ? 4u : 0u;
        if (fixed > bs - p) { loud |= LOUD_MALFORMED; break; }
        bool is_int = true, drop = false;
        int64_t iv = 0;
        switch (ty) {
        case 'A': is_int = false; p += 1u; break;
        case 'c': iv = (int8_t)d[p]; p += 1u; break;
        case 'C': iv = d[p]; p += 1u; break;
        case 's': iv = (int16_t)rd16(d + p); p += 2u; break;
        case 'S': iv = (int64_t)rd16(d + p); p += 2u; break;
        case 'i': iv = (int32_t)rd32(d + p); p += 4u; break;
        case 'I': iv = (int64_t)rd32(d + p); p += 4u; break;
        case 'Z': {
            is_int = false;
            const uint32_t v0 = p;
            bool tab = false;
            while (p < bs && d[p]) { if (d[p] == '\t') tab = true; ++p; }
            if (p >= bs) { loud |= LOUD_MALFORMED; p = bs + 1u; break; }
            if (p == v0 || tab) loud |= LOUD_Z;
            // a token whose text holds NH:i: or XS:i: anywhere is dropped (:587-589); XS:A: anywhere keeps the strand tag away (:591)
            if (holds(d + v0, p - v0, "NH:i:") || holds(d + v0, p - v0, "XS:i:")) drop = true;
            if (holds(d + v0, p - v0, "XS:A:")) xs_found = true;
            ++p;
            break; }
        default: loud |= LOUD_TAGTYPE; p = bs + 1u; is_int = false; break;      // f, d, H, B: not taken
        }
        if (p > bs) break;
        const bool is_as = k0 == 'A' && k1 == 'S';                // strncmp(tok, "AS", 2), :703: whatever its type
        if (is_as) {
            const int64_t v = s.score < 0 ? (int64_t)s.score : 0;         // AS:i:min(0, score)
            char nty; uint32_t nlen;
            int_type(v, nty, nlen);
            if (is_int && nty == ty && v == iv) { if (run_len && run_at + run_len == p0) run_len += p - p0; else { out.copy(o, d + run_at, run_len); o += run_len; run_at = p0; run_len = p - p0; } continue; }
            out.copy(o, d + run_at, run_len); o += run_len; run_len = 0;
            o = put_int_tag(out, o, k0, k1, v);
            continue;
        }
        if (is_int) {
            if ((k0 == 'N' && k1 == 'H') || (k0 == 'X' && k1 == 'S')) continue;      // its text is NH:i:... / XS:i:...
            char nty; uint32_t nlen;
            int_type(iv, nty, nlen);
            if (nty != ty) {
                out.copy(o, d + run_at, run_len); o += run_len; run_len = 0;
                o = put_int_tag(out, o, k0, k1, iv);
                continue;
            }
        } else if (ty == 'A') {
            if (k0 == 'X' && k1 == 'S') xs_found = true;           // its text is XS:A:.
        } else if (drop) continue;
        if (run_len && run_at + run_len == p0) run_len += p - p0;
        else { out.copy(o, d + run_at, run_len); o += run_len; run_at = p0; run_len = p - p0; }
    }
    out.copy(o, d + run_at, run_len); o += run_len;
    // add_auxData's own, then --rg-id (:595-653, :742-772)
    o = put_int_tag(out, o, 'N', 'H', (int64_t)s.n);
    if (s.flags & SLOT_HAS_NEXT) {
        out.put(o, (uint32_t)'C' | ((uint32_t)'C' << 8) | ((uint32_t)'Z' << 16), 3u); o += 3u;
        if (s.next_ref == s.ref_id) { out.put(o, (uint32_t)'=', 1u); o += 1u; }
        else if (s.next_ref >= 1u && s.next_ref <= (uint32_t)cfg.n_ref) {
            const uint32_t a = cfg.name_off[s.next_ref - 1u], l = cfg.name_off[s.next_ref] - a;
            out.copy(o, cfg.names + a, l); o += l;
        } else loud |= LOUD_CONTIG;
        out.put(o, 0u, 1u); o += 1u;
        o = put_int_tag(out, o, 'C', 'P', (int64_t)s.next_left + 1);
    }
    if (!xs_found && (cfg.library_type == LIB_FR_FIRSTSTRAND || cfg.library_type == LIB_FR_SECONDSTRAND)) {
        const bool anti = (flag & 0x10u) != 0u;                 // antisense_align()
        const char strand = xs_strand(cfg.library_type, anti, m.side);
        out.put(o, (uint32_t)'X' | ((uint32_t)'S' << 8) | ((uint32_t)'A' << 16) | ((uint32_t)(uint8_t)strand << 24), 4u); o += 4u;
    }
    if (s.n > 1u) o = put_int_tag(out, o, 'H', 'I', (int64_t)s.place);
    if (cfg.rg_len) {
        out.put(o, (uint32_t)'R' | ((uint32_t)'G' << 8) | ((uint32_t)'Z' << 16), 3u); o += 3u;
        out.copy(o, cfg.rg, cfg.rg_len); o += cfg.rg_len;
        out.put(o, 0u, 1u); o += 1u;
    }
    out.put(0u, o - 4u, 4u);
    if (o > 65536u) loud |= LOUD_BIG;
    return o;
}

// pairs: the pass that writes the records of inserts (its inputs are the two sides' single-end records)
THJ_HD const char* loud_text(uint32_t loud, bool pairs = false) {
    return loud & LOUD_ORDER ? "the pieces do not line up with the add calls of this consensus (the record count or the read runs differ)"
         : loud & LOUD_MALFORMED ? "a malformed record (its header, its cigar or a tag does not fit it, or a cigar operation above 8)"
         : loud & LOUD_PAIRED ? (pairs ? "an input record that already has a mate (a mate contig or flag 0x1): the sides of an insert are given as single-end records"
                                       : "paired records: not built (a record with a mate contig or flag 0x1)")
         : loud & LOUD_FUSION ? "a reported fusion alignment (XF:Z, two records): not built"
         : loud & LOUD_TAGTYPE ? "a tag of type f, d, H or B: not taken"
         : loud & LOUD_Z ? "a Z tag with an empty value, or with a TAB in it"
         : loud & LOUD_LSEQ0 ? "a record without bases (l_seq == 0)"
         : loud & LOUD_QLEN ? "a record whose cigar and SEQ differ in length"
         : loud & LOUD_CONTIG ? "a contig without an @SQ line in the output header"
         : loud & LOUD_BIG ? "a rewritten record over 64 KiB" : "";
}

}  // namespace acc

// ---- the host's share (plain functions; the kernels call none of them)
#include <math.h>
#include <algorithm>
#include <vector>
namespace acc {
// MAPQ by the reference's own expression (:734-738): 50, 3, 1, 1, 0 for n = 1 .. 5, and 0 from there on (the expression falls with n)
inline void mapq_table(uint8_t* t /*[8]*/) {
    for (int n = 0; n < 8; ++n) t[n] = 0;
    t[1] = 50;
    for (int n = 2; n <= 5; ++n) { const double err_prob = 1 - (1.0 / n); t[n] = (uint8_t)(int)(-10.0 * log(err_prob) / log(10.0)); }
}
// index_vector of a read of more than SORT_BY_COUNTING alignments: std::sort itself over 0 .. n - 1 under lex_hit_sort, which is no
// stable sort there -- the order of ties is libstdc++'s.  ref / left in `hits` order.
inline std::vector<uint32_t> sort_places(const std::vector<uint32_t>& ref, const std::vector<int32_t>& left) {
    std::vector<uint32_t> iv(ref.size());
    for (size_t i = 0; i < iv.size(); ++i) iv[i] = (uint32_t)i;
    std::sort(iv.begin(), iv.end(), [&](const uint32_t& l, const uint32_t& r) { return ref[l] != ref[r] ? ref[l] < ref[r] : left[l] < left[r]; });
    return iv;
}
}  // namespace acc
