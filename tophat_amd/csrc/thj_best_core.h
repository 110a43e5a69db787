// thj_best_core.h -- tophat_reports' choice among the alignments of one read, the single-end half:
//
//   BowtieHit::operator<, read_len(), right()            bwt_map.h:145-165, :180-207, :213-243
//   cmp_read_equal, read_best_alignments (both modes)    tophat_reports.cpp:94-111, :113-208
//   AlignStatus: the score of one alignment              align_status.cpp:40-284
//   boost::mt19937, seeded 1 per worker                  tophat_reports.cpp:2325, :1005-1007
//
// Plain functions without memory of their own: thj_juncbed_best_impl.h runs them in its kernels and in the host part of
// thj_juncbed_finish, tests/bestsim compiles them for the CPU.
//
// A read = the kept records that follow each other under one read number.  First pass: the records under the read filter's limits,
// sorted by less(), std::unique by equal() -- only the survivors feed the first-pass junction statistics.  Second pass, from the raw
// records again: limits, exclude_hits_on_filtered_junctions, score; the records at the maximum, sorted and made unique again; if more
// than max_multihits are left, none (--suppress-hits) or the survivors of trim().
//
// Pairs: thj_pair_core.h.  Not here: realign_reads, --report-secondary-alignments, and the score of a record
// without AS:i (bwt_map.cpp:1287-1292, :1377-1405: it needs MD and the qualities).
#pragma once
#include <stdint.h>
#include "thj_jb_walk.h"
#include "thj_jbknown_core.h"

namespace jbb {

// the fields operator< and cmp_read_equal compare (the read id is equal within a read); ref_id2 of an alignment without a fusion op is
// its ref_id (HitFactory::create_hit, bwt_map.cpp:284-288)
struct Key { uint32_t ref_id, ref_id2; int32_t left, right; uint8_t anti, mismatches, edit_dist, n_cigar; };

template <class CG>
THJ_HD Key key_of(uint32_t ref_id, int32_t left, bool antisense_align, uint32_t mismatches, int n_cigar, CG cg) {
    bool fused = false;
    for (int c = 0; c < n_cigar; ++c) { const uint32_t op = cg(c) >> 28; if (op >= 7u && op <= 10u) fused = true; }
    Key k;
    k.ref_id = ref_id; k.ref_id2 = fused ? cg(15) : ref_id; k.left = left;
    k.right = (int32_t)jbw::unsplit_span(n_cigar, left, cg).right;
    k.anti = antisense_align ? 1 : 0; k.mismatches = (uint8_t)mismatches;
    k.edit_dist = (uint8_t)(mismatches + jbk::gap_length(n_cigar, cg));      // bwt_map.cpp:1429-1430
    k.n_cigar = (uint8_t)n_cigar;
    return k;
}

// BowtieHit::operator< (bwt_map.h:180-207): ref_id, ref_id2, left, antisense_align, mismatches, edit_dist, cigar size, the cigar op
// by op (opcode, then length)
template <class CA, class CB>
THJ_HD bool less(const Key& a, CA ca, const Key& b, CB cb) {
    if (a.ref_id != b.ref_id) return a.ref_id < b.ref_id;
    if (a.ref_id2 != b.ref_id2) return a.ref_id2 < b.ref_id2;
    if (a.left != b.left) return a.left < b.left;
    if (a.anti != b.anti) return a.anti < b.anti;
    if (a.mismatches != b.mismatches) return a.mismatches < b.mismatches;
    if (a.edit_dist != b.edit_dist) return a.edit_dist < b.edit_dist;
    if (a.n_cigar != b.n_cigar) return a.n_cigar < b.n_cigar;
    for (int c = 0; c < a.n_cigar; ++c) {
        const uint32_t x = ca(c), y = cb(c);
        if (x != y) return (x >> 28) < (y >> 28) || ((x >> 28) == (y >> 28) && (x & jbw::LEN_MASK) < (y & jbw::LEN_MASK));
    }
    return false;
}

// cmp_read_equal (tophat_reports.cpp:94-111): right instead of the cigar, and no score
THJ_HD bool equal(const Key& a, const Key& b) {
    return a.ref_id == b.ref_id && a.ref_id2 == b.ref_id2 && a.left == b.left && a.right == b.right && a.anti == b.anti &&
           a.mismatches == b.mismatches && a.edit_dist == b.edit_dist && a.n_cigar == b.n_cigar;
}

template <class CG> THJ_HD uint32_t read_len(int n_cigar, CG cg) { return jbw::unsplit_span(n_cigar, 0, cg).read_len; }
THJ_HD int min_extent(uint32_t read_len) { const int q = (int)(read_len / 4u); return q < 10 ? q : 10; }       // align_status.cpp:56

// The junctions AlignStatus asks about, f(left, right) per REF_SKIP / rEF_SKIP in cigar order (align_status.cpp:59-85, :144-172,
// :271-278).  Its own walk: the contig is ALWAYS the alignment's first (junc.refid = bh.ref_id(), also behind a fusion op), and all
// four fusion ops -- FUSION_RR too -- set the position to the op's length.  Returns their number, which is jbw::juncs' number.
template <class CG, class F>
THJ_HD int score_juncs(int n_cigar, int32_t left0, CG cg, F f) {
    int n = 0;
    int32_t j = left0;
    for (int c = 0; c < n_cigar; ++c) {
        const uint32_t op = cg(c) >> 28; const int32_t len = (int32_t)(cg(c) & jbw::LEN_MASK);
        if (op == 11u) { f((uint32_t)(j - 1), (uint32_t)(j + len)); j += len; ++n; }
        else if (op == 12u) { f((uint32_t)(j - len), (uint32_t)(j + 1)); j -= len; ++n; }
        else if (op == 1u || op == 5u) j += len;
        else if (op == 2u || op == 6u) j -= len;
        else if (op >= 7u && op <= 10u) j = len;
    }
    return n;
}

// what the first pass knows of one such junction: found = it is in the first-pass set (a record of the first pass shows it, or the
// annotation holds it); annotated = gtf_junctions.find succeeds
struct Seen { bool found, annotated; uint32_t support, left_extent, right_extent; };

// penalty of a junction of the first-pass set that the annotation does not hold (align_status.cpp:99-122).  avg_cov is 0: the
// consensus worker's update_coverage calls are commented out (tophat_reports.cpp:2015, :2037), Coverage stays empty.  "penalty *=
// float" truncates: max_penalty 5 and a short extent give (int)(7 * 0.5f) = 3.  (The gtf_match branch, :118-119, cannot be reached:
// gtf_match is set for exactly the junctions gtf_junctions.find finds, and those took the + 2 branch.)
THJ_HD int penalty(int max_penalty, uint32_t support, uint32_t left_extent, uint32_t right_extent, int min_ext) {
    int p = max_penalty + 2;
    if ((int)support >= 5) {
        const float extent_penalty = ((int)left_extent < min_ext || (int)right_extent < min_ext) ? 0.5f : 0.0f;
        const float f = 0.0f / (float)(int)support + extent_penalty;
        p = (int)((float)p * (f < 1.f ? f : 1.f));
    }
    return p;
}

// one junction's share of the score (align_status.cpp:90-139)
THJ_HD int score_step(int score, const Seen& s, int max_penalty, int min_ext) {
    if (s.annotated) return score + 2;
    if (!s.found) return score - max_penalty;
    return score - penalty(max_penalty, s.support, s.left_extent, s.right_extent, min_ext);
}

// AlignStatus over one alignment: look(k, left, right) -> Seen for its k-th junction (the contig is the alignment's ref_id).  The
// indel branches are dead (recalculate_indel_score = false).
template <class CG, class L>
THJ_HD int score(int alignment_score, int n_cigar, int32_t left, int max_penalty, CG cg, L look) {
    const int me = min_extent(read_len(n_cigar, cg));
    int sc = alignment_score, k = 0;
    score_juncs(n_cigar, left, cg, [&](uint32_t l, uint32_t r) { sc = score_step(sc, look(k++, l, r), max_penalty, me); });
    return sc;
}

// the cap (tophat_reports.cpp:180-206) over n tied alignments, alive[0 .. n) all 1 on entry: tie_indexes = 0 .. n - 1; while more than
// max_multihits are left, erase tie_indexes[draw() % size].  The survivors keep their order.
template <class D>
THJ_HD void trim(uint32_t n, uint32_t max_multihits, D draw, uint8_t* alive) {
    for (uint32_t left = n; left > max_multihits; --left) {
        uint32_t at = (uint32_t)(draw() % left);
        for (uint32_t i = 0; i < n; ++i) if (alive[i]) { if (!at) { alive[i] = 0; break; } --at; }
    }
}

// boost::mt19937 = the standard MT19937 (seed 1: 1791095845, 4282876139, 3093770124, 4005303368, ...)
struct Mt19937 {
    uint32_t s[624]; int at;
    THJ_HD void seed(uint32_t v) { s[0] = v; for (int i = 1; i < 624; ++i) s[i] = 1812433253u * (s[i - 1] ^ (s[i - 1] >> 30)) + (uint32_t)i; at = 624; }
    THJ_HD uint32_t next() {
        if (at >= 624) {
            for (int i = 0; i < 624; ++i) {
                const uint32_t y = (s[i] & 0x80000000u) | (s[(i + 1) % 624] & 0x7FFFFFFFu);
                s[i] = s[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908B0DFu : 0u);
            }
            at = 0;
        }
        uint32_t y = s[at++];
        y ^= y >> 11; y ^= (y << 7) & 0x9D2C5680u; y ^= (y << 15) & 0xEFC60000u; y ^= y >> 18;
        return y;
    }
    THJ_HD void discard(unsigned long long n) { while (n--) (void)next(); }
};

// The generator's walk over the reads in input order (tophat_reports.cpp:170-208, :1005-1007): a read over the cap draws once per
// erased entry, and every read of which anything is reported draws once more (print_sam_for_single: rng() % hits.size(): the primary
// alignment of accepted_hits.bam; kept on request).
// The walker is told, per read over the cap in order, how many reads that report anything came before it since the last such read.
struct CapWalk {
    Mt19937 rng;
    THJ_HD void begin() { rng.seed(1u); }
    // n tied alignments of the next read over the cap, `before` reporting reads since the last one (that one not counted): alive[] as trim()
    // kept (or null): the print_sam_for_single draws are kept, not thrown away -- kept[k] for the k-th of the `before` reads, kept[before] its own
    THJ_HD void read(unsigned long long before, uint32_t n, uint32_t max_multihits, uint8_t* alive, uint32_t* kept = nullptr) {
        if (kept) for (unsigned long long k = 0; k < before; ++k) kept[k] = rng.next();
        else rng.discard(before);
        trim(n, max_multihits, [this]() { return rng.next(); }, alive);
        const uint32_t own = rng.next();                      // its own print_sam_for_single draw (max_multihits >= 1: something is left)
        if (kept) kept[before] = own;
    }
    // the reporting reads behind the last read over the cap
    THJ_HD void rest(unsigned long long n, uint32_t* kept) { for (unsigned long long k = 0; k < n; ++k) kept[k] = rng.next(); }
};

}  // namespace jbb
