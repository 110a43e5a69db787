// thj_jb_walk.h -- the record walkers of tophat_reports' consensus pass: what one reported alignment contributes to the
// JunctionSet, the DeletionSet and the InsertionSet, and (jbw::fusion, jbw::unsplit_span, further down) to the FusionSet.  Plain functions over a cigar and a callback: no atomics, no memory of their
// own; thj_juncbed_impl.h runs them on the device, tests/indelsim compiles them for the CPU.
//
//   junctions_from_spliced_hit     junctions.cpp:19-92
//   deletions_from_spliced_hit     deletions.cpp:83-151
//   insertions_from_spliced_hit    insertions.cpp:109-180
//
// Each of the three follows its own source: they do not agree on how a dEL moves the genome position (the junction and insertion walkers
// go down, the deletion walker goes UP, deletions.cpp:133), and only the insertion walker tracks a position in the read.
//
// A cigar is read through cg(c) = (op << 28) | length, op = CigarOpCode (bwt_map.h:36-55):
//   1 MATCH  2 mATCH  3 INS  4 iNS  5 DEL  6 dEL  7 FUSION_FF  8 FUSION_FR  9 FUSION_RF  10 FUSION_RR  11 REF_SKIP  12 rEF_SKIP
// everything else (clips, pads) is the `default:` of the reference's switches.  ref2 = the second contig of a fusion alignment.
// After FF / FR / RF the position jumps to the op's length and what follows lies on ref2; FUSION_RR has no case in any of the three.
#pragma once
#include <cstdint>

#ifndef THJ_WALK_FN
#if defined(__HIPCC__) || defined(__CUDACC__)
#define THJ_WALK_FN __host__ __device__ inline
#else
#define THJ_WALK_FN inline
#endif
#endif

namespace jbw {

static constexpr uint32_t LEN_MASK = 0x0FFFFFFFu;

// f(ref_id, left, right, left_extent, right_extent) per REF_SKIP / rEF_SKIP; returns their number.  Pieces that run down the genome
// walk backwards and swap the extents.
template <class CG, class F>
THJ_WALK_FN int juncs(int n_cigar, int32_t left0, uint32_t ref_id, uint32_t ref2, CG cg, F f) {
    int n = 0;
    int64_t j = left0;
    uint32_t ref = ref_id;
    for (int c = 0; c < n_cigar; ++c) {
        const uint32_t op = cg(c) >> 28, len = cg(c) & LEN_MASK;
        if (op == 11 || op == 12) {
            const uint32_t prev = c > 0 ? (cg(c - 1) & LEN_MASK) : 0u, next = c + 1 < n_cigar ? (cg(c + 1) & LEN_MASK) : 0u;
            if (op == 11) { f(ref, (uint32_t)(j - 1), (uint32_t)(j + len), prev, next); j += len; }
            else { f(ref, (uint32_t)(j - len), (uint32_t)(j + 1), next, prev); j -= len; }
            ++n;
        } else if (op == 1 || op == 5) j += len;
        else if (op == 2 || op == 6) j -= len;
        else if (op == 7 || op == 8 || op == 9) { j = len; ref = ref2; }
    }
    return n;
}

// f(ref_id, left, right, left_extent, right_extent, op index) per DEL / dEL; returns their number.
//   DEL: left = pos - 1, right = pos + len.   dEL: left = pos - len, right = pos + 1 -- and the position then goes UP by len for both
//   (deletions.cpp:115-133).  Extents: the lengths of the ops before and after, not swapped.  Unsigned 32-bit arithmetic as there.
template <class CG, class F>
THJ_WALK_FN int dels(int n_cigar, int32_t left0, uint32_t ref_id, uint32_t ref2, CG cg, F f) {
    int n = 0;
    uint32_t pos = (uint32_t)left0, ref = ref_id;
    for (int c = 0; c < n_cigar; ++c) {
        const uint32_t op = cg(c) >> 28, len = cg(c) & LEN_MASK;
        if (op == 11 || op == 1) pos += len;
        else if (op == 12 || op == 2) pos -= len;
        else if (op == 5 || op == 6) {
            const uint32_t prev = c > 0 ? (cg(c - 1) & LEN_MASK) : 0u, next = c + 1 < n_cigar ? (cg(c + 1) & LEN_MASK) : 0u;
            if (op == 5) f(ref, pos - 1u, pos + len, prev, next, c);
            else f(ref, pos - len, pos + 1u, prev, next, c);
            pos += len;
            ++n;
        } else if (op == 7 || op == 8 || op == 9) { pos = len; ref = ref2; }
    }
    return n;
}

// f(ref_id, left, length, position in the read, left_extent, right_extent, op index) per INS / iNS; returns their number.
//   INS: left = pos - 1.   iNS: left = pos + 1 (insertions.cpp:153-156).  The inserted letters are SEQ[position in the read ..
//   + length) of the record's SEQ as aligned; the position advances on MATCH, mATCH, INS and iNS only (:129, :166) -- a soft clip
//   does not move it although BAMHitFactory::get_hit_from_buf keeps the clipped bases in seq() (bwt_map.cpp:1158-1165: all l_qseq
//   bases; a fusion record: the bases field of XF:Z, :1231-1232), so behind a leading clip the letters come from in front of where
//   the aligner put them.  That is the reference's answer and the one given here.
template <class CG, class F>
THJ_WALK_FN int inss(int n_cigar, int32_t left0, uint32_t ref_id, uint32_t ref2, CG cg, F f) {
    int n = 0;
    uint32_t pos = (uint32_t)left0, ref = ref_id, rpos = 0;
    for (int c = 0; c < n_cigar; ++c) {
        const uint32_t op = cg(c) >> 28, len = cg(c) & LEN_MASK;
        if (op == 11 || op == 5) pos += len;
        else if (op == 12 || op == 6) pos -= len;
        else if (op == 1) { pos += len; rpos += len; }
        else if (op == 2) { pos -= len; rpos += len; }
        else if (op == 3 || op == 4) {
            const uint32_t prev = c > 0 ? (cg(c - 1) & LEN_MASK) : 0u, next = c + 1 < n_cigar ? (cg(c + 1) & LEN_MASK) : 0u;
            f(ref, op == 3 ? pos - 1u : pos + 1u, len, rpos, prev, next, c);
            rpos += len;
            ++n;
        } else if (op == 7 || op == 8 || op == 9) { pos = len; ref = ref2; }
    }
    return n;
}

// the fusion of one record and its anchors, in one pass over the cigar: fusions_from_spliced_hit with auto_sort (fusions.cpp:441-495) and
// the left / right sums of fusions_from_alignment (:141-194).  Unlike the three walkers above this one has a case for FUSION_RR.
//   key walk: MATCH, REF_SKIP, DEL go up, their lower-case forms down (unsigned 32-bit, it may wrap below 0); at the fusion op the
//   position steps back by one for FF / FR and forward by one for RF / RR.  key = (ref, ref2, position, op length, dir) when
//   ref < ref2, or the contigs are equal and position < length; else contigs and coordinates swap, dir stays.
//   left_pos / right_pos: the MATCH, REF_SKIP and DEL lengths (either case) before / after the op.  inner: the op is neither the first
//   nor the last of the cigar -- fusions_from_alignment drops the others.  Only the first fusion op of a cigar is looked at (a record
//   holds one: its second contig is a single field).
struct FusionSite { uint32_t ref1, ref2, left, right, dir, left_pos, right_pos; bool inner; };
template <class CG>
THJ_WALK_FN bool fusion(int n_cigar, int32_t left0, uint32_t ref_id, uint32_t ref2, CG cg, FusionSite& s) {
    uint32_t pos = (uint32_t)left0, lsum = 0, rsum = 0;
    int at = -1;
    for (int c = 0; c < n_cigar; ++c) {
        const uint32_t op = cg(c) >> 28, len = cg(c) & LEN_MASK;
        const bool up = op == 1 || op == 11 || op == 5, down = op == 2 || op == 12 || op == 6;
        if (at >= 0) { if (up || down) rsum += len; continue; }
        if (up) { pos += len; lsum += len; }
        else if (down) { pos -= len; lsum += len; }
        else if (op >= 7 && op <= 10) {
            at = c;
            const uint32_t p = (op == 9 || op == 10) ? pos + 1u : pos - 1u;
            s.dir = op;
            if (ref_id < ref2 || (ref_id == ref2 && p < len)) { s.ref1 = ref_id; s.ref2 = ref2; s.left = p; s.right = len; }
            else { s.ref1 = ref2; s.ref2 = ref_id; s.left = len; s.right = p; }
        }
    }
    if (at < 0) return false;
    s.left_pos = lsum; s.right_pos = rsum; s.inner = at > 0 && at + 1 < n_cigar;
    return true;
}

// what unsupport_fusions asks of a record (fusions.cpp:287-295): read_len() (bwt_map.h:145-165: MATCH, mATCH, INS, iNS, SOFT_CLIP),
// right() (:213-243) and whether it qualifies: no fusion op, no REF_SKIP / rEF_SKIP, read_len() >= 40
struct UnsplitSpan { uint32_t read_len, right; bool qualifies; };
template <class CG>
THJ_WALK_FN UnsplitSpan unsplit_span(int n_cigar, int32_t left0, CG cg) {
    uint32_t rl = 0, r = (uint32_t)left0;
    bool plain = true;
    for (int c = 0; c < n_cigar; ++c) {
        const uint32_t op = cg(c) >> 28, len = cg(c) & LEN_MASK;
        if (op == 1 || op == 2 || op == 3 || op == 4 || op == 13) rl += len;
        if (op == 1 || op == 11 || op == 5) r += len;
        else if (op == 2 || op == 12 || op == 6) r -= len;
        else if (op >= 7 && op <= 10) r = len;
        if ((op >= 7 && op <= 12)) plain = false;
    }
    return UnsplitSpan{rl, r, plain && rl >= 40u};
}

// the same over a plain cigar array of 16 words (thj_aln: ref_id2 of a fusion alignment in cigar[15])
struct ArrayCigar { const uint32_t* w; THJ_WALK_FN uint32_t operator()(int c) const { return w[c]; } };
template <class F> THJ_WALK_FN int juncs(const uint32_t* cigar, int n_cigar, int32_t left, uint32_t ref_id, F f) { return juncs(n_cigar, left, ref_id, cigar[15], ArrayCigar{cigar}, f); }
template <class F> THJ_WALK_FN int dels(const uint32_t* cigar, int n_cigar, int32_t left, uint32_t ref_id, F f) { return dels(n_cigar, left, ref_id, cigar[15], ArrayCigar{cigar}, f); }
template <class F> THJ_WALK_FN int inss(const uint32_t* cigar, int n_cigar, int32_t left, uint32_t ref_id, F f) { return inss(n_cigar, left, ref_id, cigar[15], ArrayCigar{cigar}, f); }
THJ_WALK_FN bool fusion(const uint32_t* cigar, int n_cigar, int32_t left, uint32_t ref_id, FusionSite& s) { return fusion(n_cigar, left, ref_id, cigar[15], ArrayCigar{cigar}, s); }
THJ_WALK_FN UnsplitSpan unsplit_span(const uint32_t* cigar, int n_cigar, int32_t left) { return unsplit_span(n_cigar, left, ArrayCigar{cigar}); }

}  // namespace jbw
