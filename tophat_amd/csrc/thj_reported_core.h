// thj_reported_core.h -- one BAM record of a file of REPORTED alignments (a spanning BAM of long_spanning_reads, a whole-read map,
// an accepted_hits file) -> one thj_aln for the junction consensus (thj_juncbed_*), or nothing: what thj_junctions' host reader does
// per record (host/thj_junctions_main.cpp: parse_record and keep), decision for decision and in the same order.  A fusion alignment
// comes as two records that both carry the whole alignment in XF:Z ("1|2 <contig1>-<contig2> <pos> <cigar with an F op> <bases>
// <qualities>", print_bamhit, bwt_map.cpp:2047-2083): the first is rebuilt from the tag the way BAMHitFactory::get_hit_from_buf
// does (bwt_map.cpp:1208-1318), the second is dropped.
// Plain per-record functions without memory of their own: thj_k_parse_reported (thj_ingest.hip) calls them per thread,
// tests/reportedsim compiles them for the CPU.  A record starts at any byte address, so every field is put together from byte loads.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/thj.h"
#include "thj_jb_walk.h"
#include "thj_jbknown_core.h"

#ifndef THJ_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define THJ_HD __host__ __device__ __forceinline__
#else
#define THJ_HD inline
#endif
#endif

namespace rpt {

// what a record can report beside "kept" / "dropped": the host reader ends the run at each of these
enum { REP_MALFORMED = 1u,      // the header, a tag or an array tag does not fit the record
       REP_XF_OPS = 2u,         // a fusion alignment of more than 15 CIGAR operations
       REP_CIGAR = 4u,          // a kept alignment of more than 16 CIGAR operations
       REP_INS_RANGE = 8u,      // an insertion that lies outside the record's bases
       REP_INS_LONG = 16u,      // an insertion of more than 16 bases
       REP_INS_LETTER = 32u,    // an inserted letter other than A, C, G, T, N
       REP_NO_AS = 64u };       // best alignments are chosen and a kept record has no AS:i, or one outside int16: no score is guessed
static constexpr uint32_t MAX_INS = 16;

// the run's contig names: names[r] = blob[off[r] .. off[r + 1]), ref_id = r + 1; sorted[] = 0 .. n - 1 ordered by (name bytes, r)
struct Names { const uint8_t* blob; const uint32_t* off; const uint32_t* sorted; int32_t n; };
// best: thj_aln.AS is needed (REP_NO_AS); whoever sets it sets fusions too -- every mapped record on a known contig is kept
struct Cfg { const uint32_t* tid2ref; uint32_t n_tid; int32_t max_report_intron; bool indels, fusions; Names names; bool best = false; };
// where seq() of a kept record lies inside it: the 4-bit SEQ, or (a fusion record) the ASCII bases of its tag
struct Seq { uint32_t at, len; bool ascii; };

THJ_HD uint32_t rd16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
THJ_HD uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// RefTable::get_id of a frozen table for name[0 .. len): bisection over the sorted permutation; 0 = no such contig
THJ_HD uint32_t name_id(const Names& nm, const uint8_t* name, uint32_t len) {
    int32_t lo = 0, hi = nm.n;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        const uint32_t r = nm.sorted[mid], a = nm.off[r], l = nm.off[r + 1] - a, m = l < len ? l : len;
        int c = 0;
        for (uint32_t k = 0; k < m && !c; ++k) c = (int)nm.blob[a + k] - (int)name[k];
        if (!c) c = l < len ? -1 : l > len ? 1 : 0;
        if (c < 0) lo = mid + 1; else hi = mid;
    }
    if (lo >= nm.n) return 0;
    const uint32_t r = nm.sorted[lo], a = nm.off[r];
    if (nm.off[r + 1] - a != len) return 0;
    for (uint32_t k = 0; k < len; ++k) if (nm.blob[a + k] != name[k]) return 0;
    return r + 1;
}

// strtol(s + i, &t, 10) over text that ends at e: white space, a sign, digits; saturates; i moves behind the digits (stays when
// there are none)
THJ_HD int64_t dec_long(const uint8_t* s, uint32_t& i, uint32_t e) {
    uint32_t k = i;
    while (k < e && (s[k] == ' ' || (s[k] >= 9 && s[k] <= 13))) ++k;
    bool neg = false;
    if (k < e && (s[k] == '+' || s[k] == '-')) { neg = s[k] == '-'; ++k; }
    if (k >= e || s[k] < '0' || s[k] > '9') return 0;
    uint64_t v = 0;
    const uint64_t lim = neg ? (uint64_t)1 << 63 : ((uint64_t)1 << 63) - 1;
    for (; k < e && s[k] >= '0' && s[k] <= '9'; ++k) {
        const uint64_t dg = (uint64_t)(s[k] - '0');
        v = v > (lim - dg) / 10 ? lim : v * 10 + dg;
    }
    i = k;
    return neg ? (int64_t)(0 - v) : (int64_t)v;
}

// letter k of a kept record's seq()
THJ_HD char seq_letter(const uint8_t* d, const Seq& s, uint32_t k) {
    if (s.ascii) return (char)d[s.at + k];
    return "=ACMGRSVTWYHKDBN"[(d[s.at + (k >> 1)] >> ((~k & 1u) << 2)) & 15u];
}

// the inserted letters of kept record `a`: their number, and what the host reader and the add call end the run for
THJ_HD uint32_t ins_check(const uint8_t* d, const thj_aln& a, const Seq& s, uint32_t& rep) {
    uint32_t n = 0;
    jbw::inss(a.cigar, a.n_cigar, a.left, a.ref_id, [&](uint32_t, uint32_t, uint32_t len, uint32_t rpos, uint32_t, uint32_t, int) {
        if ((uint64_t)rpos + len > (uint64_t)s.len) { rep |= REP_INS_RANGE; return; }
        if (len > MAX_INS) rep |= REP_INS_LONG;
        for (uint32_t k = 0; k < len; ++k) {
            const char ch = seq_letter(d, s, rpos + k);
            if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T' && ch != 'N') rep |= REP_INS_LETTER;
        }
        n += len;
    });
    return n;
}
// ... and the letters themselves, op after op in cigar order (a record ins_check found nothing to report for)
THJ_HD void ins_letters(const uint8_t* d, const thj_aln& a, const Seq& s, uint8_t* out) {
    uint32_t n = 0;
    jbw::inss(a.cigar, a.n_cigar, a.left, a.ref_id, [&](uint32_t, uint32_t, uint32_t len, uint32_t rpos, uint32_t, uint32_t, int) {
        for (uint32_t k = 0; k < len; ++k) out[n++] = (uint8_t)seq_letter(d, s, rpos + k);
    });
}

// --fusions-out: do two records belong to one read?  QNAME (up to l_read_name, cut at the first NUL) and the 0x40 / 0x80 bits
THJ_HD bool same_read(const uint8_t* x, const uint8_t* y) {
    if (((rd32(x + 12) ^ rd32(y + 12)) >> 22) & 3u) return false;
    const uint32_t lx = x[8], ly = y[8];
    for (uint32_t k = 0;; ++k) {
        const bool ex = k >= lx || !x[32 + k], ey = k >= ly || !y[32 + k];
        if (ex || ey) return ex && ey;
        if (x[32 + k] != y[32 + k]) return false;
    }
}

// record d (after its block_size field, bs bytes) -> a; false = nothing (rep says whether loudly).  s / n_ins: of a kept record
THJ_HD bool reported_record(const uint8_t* d, uint32_t bs, const Cfg& cfg, thj_aln& a, Seq& s, uint32_t& n_ins, uint32_t& rep) {
    n_ins = 0; s.at = 0; s.len = 0; s.ascii = false;
    if (bs < 32u) { rep |= REP_MALFORMED; return false; }
    const int32_t tid = (int32_t)rd32(d), p0 = (int32_t)rd32(d + 4), l_seq = (int32_t)rd32(d + 16);
    const uint32_t flag_nc = rd32(d + 12), l_rn = d[8], n_cig = flag_nc & 0xFFFFu;
    if (l_seq < 0 || l_rn == 0u || 32ull + l_rn + 4ull * n_cig + ((uint64_t)l_seq + 1ull) / 2ull + (uint64_t)l_seq > (uint64_t)bs || d[32u + l_rn - 1u] != 0) {
        rep |= REP_MALFORMED; return false;
    }
    if (tid < 0 || ((flag_nc >> 16) & 4u)) return false;
    a.read_idx = 0; a.ref_id = 0; a.left = 0; a.flags = 0; a.mismatches = 0; a.edit_dist = 0; a.n_cigar = 0; a.AS = 0;
    a.XM = a.XO = a.XG = a.md_len = 0; a.order = 0;
    for (int i = 0; i < 16; ++i) a.cigar[i] = 0;
    for (int i = 0; i < 40; ++i) a.md[i] = 0;
    bool spliced = false, gapped = false;
    uint32_t pp = 32u + l_rn;
    for (uint32_t i = 0; i < n_cig; ++i, pp += 4) {
        const uint32_t c = rd32(d + pp), b = c & 0xFu;
        // MIDNSHP=X: = and X are matches, H and P the codes 14 and 15 the walkers pass over, anything else 15
        const uint32_t op = b == 0u || b == 7u || b == 8u ? THJ_CIG_MATCH : b == 1u ? THJ_CIG_INS : b == 2u ? THJ_CIG_DEL : b == 3u ? THJ_CIG_REF_SKIP
                          : b == 4u ? THJ_CIG_SOFT_CLIP : b == 5u ? 14u : 15u;
        if (op == THJ_CIG_REF_SKIP) spliced = true;
        if (op == THJ_CIG_INS || op == THJ_CIG_DEL) gapped = true;
        if (i < 16u) a.cigar[i] = (op << 28) | (c >> 4);
    }
    const uint32_t seq4 = pp;
    pp += ((uint32_t)l_seq + 1u) / 2u + (uint32_t)l_seq;
    char xs = 0;
    int64_t nm = 0, as = 0;                                 // AS:i like NM:i in whatever width the writer chose (bam_aux2i)
    bool has_as = false;
    uint32_t xf = 0;                                        // where the value of the last whole XF:Z lies (0: none)
    while (pp + 3u <= bs) {
        const char t0 = (char)d[pp], t1 = (char)d[pp + 1], ty = (char)d[pp + 2];
        pp += 3;
        const bool is_nm = t0 == 'N' && t1 == 'M', is_as = t0 == 'A' && t1 == 'S';
        int64_t iv = 0; bool is_int = true;
        const uint32_t fixed = (ty == 'A' || ty == 'c' || ty == 'C') ? 1u : (ty == 's' || ty == 'S') ? 2u : (ty == 'i' || ty == 'I' || ty == 'f') ? 4u : ty == 'd' ? 8u : ty == 'B' ? 5u : 0u;
        if (fixed > bs - pp) { rep |= REP_MALFORMED; return false; }
        switch (ty) {
        case 'A': if (t0 == 'X' && t1 == 'S') xs = (char)d[pp]; pp += 1; is_int = false; break;
        case 'c': iv = (int8_t)d[pp]; pp += 1; break;
        case 'C': iv = d[pp]; pp += 1; break;
        case 's': iv = (int16_t)rd16(d + pp); pp += 2; break;
        case 'S': iv = (int64_t)rd16(d + pp); pp += 2; break;
        case 'i': iv = (int32_t)rd32(d + pp); pp += 4; break;
        case 'I': iv = (int64_t)rd32(d + pp); pp += 4; break;
        case 'f': pp += 4; is_int = false; break;
        case 'd': pp += 8; is_int = false; break;
        case 'Z': case 'H': {
            const uint32_t at = pp;
            while (pp < bs && d[pp]) ++pp;
            if (pp < bs && ty == 'Z' && t0 == 'X' && t1 == 'F') xf = at;
            ++pp; is_int = false; break; }
        case 'B': {
            const char st = (char)d[pp];
            const int32_t cnt = (int32_t)rd32(d + pp + 1);
            if (cnt < 0 || (int64_t)cnt > (int64_t)bs) { rep |= REP_MALFORMED; return false; }
            const uint64_t to = (uint64_t)pp + 5u + (uint64_t)cnt * ((st == 'c' || st == 'C') ? 1u : (st == 's' || st == 'S') ? 2u : 4u);
            pp = to > (uint64_t)bs ? bs : (uint32_t)to; is_int = false; break; }
        default: pp = bs; is_int = false; break;
        }
        if (is_int && is_nm) nm = iv;
        if (is_int && is_as) { as = iv; has_as = true; }
    }
    a.flags = (uint8_t)(xs == '-' ? THJ_HIT_ANTISENSE_SPLICE : 0u);
    a.edit_dist = (uint8_t)(nm < 0 ? 0 : nm > 255 ? 255 : nm);
    if (xf) {
        if (d[xf] == '2') return false;                    // "ignore the second part of a fusion alignment" (bwt_map.cpp:1214-1216)
        // the first five fields: the non-empty runs between blanks
        uint32_t fa[5] = {0, 0, 0, 0, 0}, fe[5] = {0, 0, 0, 0, 0}, nf = 0, q = xf;
        while (d[q] && nf < 5u) {
            while (d[q] == ' ') ++q;
            if (!d[q]) break;
            const uint32_t b0 = q;
            while (d[q] && d[q] != ' ') ++q;
            fa[nf] = b0; fe[nf] = q; ++nf;
        }
        if (nf < 4u) return false;
        // the contig field's first two names: the non-empty runs between '-'
        uint32_t ca[2] = {0, 0}, ce[2] = {0, 0}, nc = 0;
        for (q = fa[1]; q < fe[1] && nc < 2u;) {
            while (q < fe[1] && d[q] == '-') ++q;
            if (q >= fe[1]) break;
            const uint32_t b0 = q;
            while (q < fe[1] && d[q] != '-') ++q;
            ca[nc] = b0; ce[nc] = q; ++nc;
        }
        if (nc < 2u) return false;                          // (the host reader looks the empty name up as the second contig: 0)
        const uint32_t r1 = name_id(cfg.names, d + ca[0], ce[0] - ca[0]), r2 = name_id(cfg.names, d + ca[1], ce[1] - ca[1]);
        if (!r1 || !r2) return false;
        uint32_t n = 0, w2 = 0, w1 = 0;                     // the two operations before the one being read
        bool spl = false, gap = false;
        for (int i = 0; i < 16; ++i) a.cigar[i] = 0;
        for (q = fa[3]; q < fe[3];) {
            const int64_t len0 = dec_long(d, q, fe[3]);
            int64_t len = len0;
            if (len <= 0) return false;
            const char ch = q < fe[3] ? (char)d[q] : (char)0;
            uint32_t code;
            switch (ch) {
            case 'M': code = 1; break; case 'm': code = 2; break; case 'I': code = 3; gap = true; break; case 'i': code = 4; gap = true; break;
            case 'D': code = 5; gap = true; break; case 'd': code = 6; gap = true; break;
            case 'N': case 'n': if (len > (int64_t)cfg.max_report_intron) return false; code = ch == 'N' ? 11u : 12u; spl = true; break;
            case 'F': code = 7; len = len - 1; break;
            case 'S': code = 13; break; case 'H': code = 14; break; case 'P': code = 15; break;
            default: return false;
            }
            ++q;
            if (n >= 15u) { rep |= REP_XF_OPS; return false; }
            const uint32_t w = code << 28 | ((uint32_t)len & 0x0FFFFFFFu);
            a.cigar[n++] = w;
            if (n >= 3u && (w1 >> 28) == 7u) {              // the direction of the fusion from the pieces around it (bwt_map.cpp:1283-1301)
                const uint32_t c2 = w2 >> 28, c0 = w >> 28;
                const bool i1 = c2 == 1u || c2 == 5u || c2 == 3u || c2 == 11u, i2 = c0 == 1u || c0 == 5u || c0 == 3u || c0 == 11u;
                const uint32_t dir = (i1 && !i2) ? 8u : (!i1 && i2) ? 9u : (!i1 && !i2) ? 10u : 7u;
                w1 = dir << 28 | (w1 & 0x0FFFFFFFu);
                a.cigar[n - 2u] = w1;
            }
            w2 = w1; w1 = w;
        }
        if (!spl && !(cfg.indels && gap) && !cfg.fusions) return false;
        a.cigar[15] = r2;
        a.ref_id = r1; a.n_cigar = (uint8_t)n;
        q = fa[2];
        a.left = (int32_t)((uint32_t)(int32_t)dec_long(d, q, fe[2]) - 1u);
        s.ascii = true; s.at = nf > 4u ? fa[4] : 0u; s.len = nf > 4u ? fe[4] - fa[4] : 0u;     // seq() of a fusion record: the tag's bases (:1231-1232)
    } else {
        if (!(spliced && n_cig >= 3u) && !(cfg.indels && gapped) && !(cfg.fusions && !spliced)) return false;
        // a spliced alignment the consensus cannot hold must not vanish from the support counts silently
        if (n_cig > 16u) { rep |= REP_CIGAR; return false; }
        a.ref_id = (uint32_t)tid < cfg.n_tid ? cfg.tid2ref[tid] : 0u;
        if (!a.ref_id) return false;
        a.left = p0; a.n_cigar = (uint8_t)n_cig;
        s.ascii = false; s.at = seq4; s.len = (uint32_t)l_seq;
    }
    // what the read filter reads (thj_jbknown_core.h): NM less the I and D of the cigar the alignment has now -- XF:Z's for a fusion alignment
    a.mismatches = jbk::mismatches(nm, (int)a.n_cigar, jbw::ArrayCigar{a.cigar});
    if (cfg.best) {
        if (!has_as || as < -32768 || as > 32767) { rep |= REP_NO_AS; return false; }
        a.AS = (int16_t)as;
        if ((flag_nc >> 16) & 0x10u) a.flags |= THJ_HIT_ANTISENSE;      // antisense_align(): BowtieHit::operator< and cmp_read_equal compare it
    }
    if (cfg.indels) {
        uint32_t r = 0;
        n_ins = ins_check(d, a, s, r);
        if (r) { rep |= r; return false; }
    }
    return true;
}

}  // namespace rpt
