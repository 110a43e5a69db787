// thj_pair_core.h -- tophat_reports' choice among the alignments of an insert, the paired half beside thj_best_core.h:
//
//   pair_distances                                        inserts.cpp:105-132
//   is_fusion_insert_alignment, set_insert_alignment_grade tophat_reports.cpp:217-261
//   InsertAlignmentGrade: the score and the too_far rescue inserts.h:72-184, operator< inserts.cpp:22-46
//   cmp_pair_alignment, cmp_pair_equal                    tophat_reports.cpp:263-294
//   pair_best_alignments (both modes), the cap            tophat_reports.cpp:358-576
//
// Plain functions without memory of their own: thj_juncbed_pair_impl.h runs them in its kernels and in the host part of the add call and of
// thj_juncbed_finish, tests/pairsim compiles them for the CPU.
//
// Only the score orders grades: with both ends mapped operator< compares alignment_score alone, so a grade is its score and whether the
// pair is a "fusion" pair.  fusion_search is false throughout (--fusion-search grading is not built): a fusion pair costs max_penalty.
//
// The list of an insert.  Candidates are generated left-major over the first 2 * max_multihits + 1 records of each side that are still
// there.  First pass (final_report false): every allowed candidate is kept, except a fusion pair when discordant pairs are not reported.
// Second pass: the reference's sequential rule, step() below.  Then std::sort by score descending -- libstdc++'s: up to 16 entries an
// insertion sort, ties stand in generation order, place16() finds every entry's place by counting; a longer list is handed to the host,
// which runs std::sort itself on the same sequence of scores with the same comparator (sort_order()), so the order is the reference's
// wherever both are built with the same libstdc++ -- then std::unique of neighbours by cmp_pair_equal, in that order.
#pragma once
#include <stdint.h>
#include "thj_best_core.h"
#include <algorithm>
#include <numeric>

namespace jbp {

// inner_dist_mean, inner_dist_std_dev (>= 1: the reference divides by it), fusion_min_dist, bowtie2_max_penalty, max_multihits
// max_report_intron: what concordant() compares the inner distance with (inserts.h:222-225); only the align-summary counters read it
struct Cfg { int32_t mean, sd, fusion_min_dist, max_penalty, max_multihits; uint8_t report_mixed, report_discordant, suppress, final_report; int32_t max_report_intron = 0; };
// what the grade reads of one alignment; score: AS in the first pass, the AlignStatus score in the second; spliced: not contiguous()
// (bwt_map.h:496-499: anything but one MATCH operation), anti_splice: antisense_splice() -- what happy() asks beside the score
struct Hit { uint32_t ref_id; int32_t left, right, score; uint8_t anti, fused, spliced, anti_splice; };

THJ_HD uint32_t side_cap(const Cfg& c) { return 2u * (uint32_t)c.max_multihits + 1u; }       // (nhits >> 1) > max_multihits ends the side

// pair_distances().second: 0 when one hit contains the other, else the start of the hit further right minus the end of the other
THJ_HD int inner_dist(const Hit& h1, const Hit& h2) {
    if (h1.left <= h2.left && h1.right >= h2.right) return 0;
    if (h2.left <= h1.left && h2.right >= h1.right) return 0;
    return h1.left < h2.left ? h2.left - h1.right : h1.left - h2.right;
}

// is_fusion_insert_alignment: a fusion op on either side, two contigs, equal strands, or the distance of the two left()s (left() on
// purpose, not right()) negative or above fusion_min_dist
THJ_HD bool is_fusion(const Hit& l, const Hit& r, int fusion_min_dist) {
    if (l.fused || r.fused) return true;
    if (l.ref_id != r.ref_id) return true;
    if (l.anti == r.anti) return true;
    const int d = l.anti ? l.left - r.left : r.left - l.left;
    return d < 0 || d > fusion_min_dist;
}
THJ_HD bool allowed(const Hit& l, const Hit& r) { return !(l.fused && r.fused); }             // set_insert_alignment_grade

// the gap a rescuing junction must lie in (inserts.h:113-117)
THJ_HD void inner_ends(const Hit& h1, const Hit& h2, int& inner1, int& inner2) {
    if (h1.left < h2.left) { inner1 = h1.right; inner2 = h2.left; } else { inner1 = h2.right; inner2 = h1.left; }
}
// one junction of h1's contig against the too_far rescue (inserts.h:127-132); support: its FIRST-pass support
THJ_HD bool rescues(int jleft, int jright, uint32_t support, int inner1, int inner2, const Cfg& c) {
    if (!(inner1 <= jleft && inner2 >= jright && support >= 10u)) return false;
    const int d = jleft - inner1 + inner2 - jright;
    return d >= c.mean - c.sd && d <= c.mean + c.sd;
}
// ... and the distance it leaves, which becomes the grade's inner_dist (inserts.h:141)
THJ_HD int rescued_dist(int jleft, int jright, int inner1, int inner2) { return jleft - inner1 + inner2 - jright; }

// InsertAlignmentGrade's alignment_score (integer arithmetic as written there).  rescue(ref_id, inner1, inner2, dist) -> some junction of the
// set handed in rescues(); dist = rescued_dist() of the FIRST such junction in the set's order (the reference breaks there, inserts.h:141-144):
// the score does not read it -- a rescued pair is neither too far nor too close -- concordant() does.
// too_far: as it stands after the rescue (what happy() reads); inner_after: the grade's inner_dist as it stands then
template <class R>
THJ_HD int grade_dist(const Hit& h1, const Hit& h2, const Cfg& c, bool fusion, R rescue, bool& too_far, int& inner_after) {
    const int min_d = c.mean - c.sd, max_d = c.mean + c.sd;
    const int inner = inner_dist(h1, h2);
    inner_after = inner;
    too_far = inner > max_d;
    const bool too_close = inner < min_d;
    if (too_far && !fusion) {
        int inner1, inner2, d = inner;
        inner_ends(h1, h2, inner1, inner2);
        if (rescue(h1.ref_id, inner1, inner2, d)) { too_far = false; inner_after = d; }
    }
    int score = h1.score + h2.score;
    if (!fusion) {
        if (too_far) score -= inner - max_d < c.sd ? c.max_penalty / 2 : c.max_penalty;
        else if (too_close) { const int a = c.max_penalty / 2, b = (min_d - inner) / c.sd + 1; score -= a < b ? a : b; }
        if (h1.anti == h2.anti) score -= c.max_penalty;
    } else score -= c.max_penalty;                               // fusion_search is false
    return score;
}
// (a rescue that only says whether: what the choice itself needs)
template <class R>
THJ_HD int grade(const Hit& h1, const Hit& h2, const Cfg& c, bool fusion, R rescue, bool& too_far) {
    int inner_after;
    return grade_dist(h1, h2, c, fusion, [&](uint32_t ref, int inner1, int inner2, int&) { return rescue(ref, inner1, inner2); }, too_far, inner_after);
}
template <class R>
THJ_HD int grade(const Hit& h1, const Hit& h2, const Cfg& c, bool fusion, R rescue) { bool too_far; return grade(h1, h2, c, fusion, rescue, too_far); }
// InsertAlignmentGrade::concordant() (inserts.h:222-225) of a pair's grade: num_mapped is 2; opposite_strands; the inner distance after the rescue
THJ_HD bool concordant(const Hit& h1, const Hit& h2, int inner_after, const Cfg& c) { return h1.anti != h2.anti && inner_after <= c.max_report_intron; }

// InsertAlignmentGrade::happy() (inserts.h:218-221) of a pair's grade: num_mapped is 2; opposite_strands; consistent_splices = both spliced
// and antisense_splice() equal (:103); too_far after the rescue.  print_sam_for_pair sets 0x2 from the insert's BEST grade.
THJ_HD bool happy(const Hit& h1, const Hit& h2, bool too_far) {
    const int num_spliced = (h1.spliced ? 1 : 0) + (h2.spliced ? 1 : 0);
    const bool consistent = num_spliced == 2 && h1.anti_splice == h2.anti_splice;
    return h1.anti != h2.anti && (num_spliced != 2 || consistent) && !too_far;
}

// The sequential rule of pair_best_alignments over the allowed candidates in generation order (tophat_reports.cpp:441-468): the running
// best rises on every allowed candidate, also on a fusion candidate that is then skipped; in the second pass a candidate that is not
// skipped and strictly raises it empties the list and enters it, one that equals it enters it -- so the list can hold different scores.
// best_happy / best_conc: happy() / concordant() of the grade the best stands at (best_grade = the first candidate in generation order that
// raised it, :443-447)
struct Running { int32_t best; uint8_t any, best_fusion, best_happy, best_conc; };
enum { STEP_SKIP = 0, STEP_ENTER = 1, STEP_CLEAR_ENTER = 2 };
THJ_HD int step(Running& r, int score, bool fusion, const Cfg& c, bool is_happy = false, bool is_conc = false) {
    bool new_best = false;
    if (!r.any || r.best < score) { r.any = 1; r.best = score; r.best_fusion = fusion ? 1 : 0; r.best_happy = is_happy ? 1 : 0; r.best_conc = is_conc ? 1 : 0; new_best = true; }
    if (fusion && !c.report_discordant) return STEP_SKIP;
    if (!c.final_report) return STEP_ENTER;
    if (new_best) return STEP_CLEAR_ENTER;
    return score < r.best ? STEP_SKIP : STEP_ENTER;
}

// place of entry a among n <= 16 entries under std::sort by score descending: an insertion sort, ties in generation order
template <class S>
THJ_HD uint32_t place16(uint32_t n, uint32_t a, S score) {
    const int32_t sa = score(a);
    uint32_t p = 0;
    for (uint32_t b = 0; b < n; ++b) { const int32_t sb = score(b); p += (sb > sa || (sb == sa && b < a)) ? 1u : 0u; }
    return p;
}
static constexpr uint32_t SORT_SMALL = 16;                        // libstdc++'s _S_threshold

// the cap (tophat_reports.cpp:538-571) over a list sorted by score descending with more than max_multihits entries: the score at place
// max_multihits - 1, the entries above it, its ties (they follow each other)
template <class S>
THJ_HD void cap_split(uint32_t n, uint32_t max_multihits, S score, uint32_t& better, uint32_t& ties) {
    const int32_t tie = score(max_multihits - 1u);
    better = ties = 0;
    for (uint32_t i = 0; i < n; ++i) { const int32_t s = score(i); if (s == tie) ++ties; else if (s < tie) break; else ++better; }
}
// ... and the draws among the ties: alive[0 .. ties) all 1 on entry; the survivors are the entries above and the ties left alive
template <class D>
THJ_HD void trim_pairs(uint32_t better, uint32_t ties, uint32_t max_multihits, D draw, uint8_t* alive) {
    for (uint32_t left = ties; better + left > max_multihits; --left) {
        uint32_t at = (uint32_t)(draw() % left);
        for (uint32_t i = 0; i < ties; ++i) if (alive[i]) { if (!at) { alive[i] = 0; break; } --at; }
    }
}

// host only: std::sort with cmp_pair_alignment over a list of these scores: order[place] = the entry that comes to stand there
inline void sort_order(const int32_t* score, uint32_t n, uint32_t* order) {
    std::iota(order, order + n, 0u);
    std::sort(order, order + n, [score](uint32_t l, uint32_t r) { return score[r] < score[l]; });
}

}  // namespace jbp
