// thj_jb_walk.h -- the three record walkers of tophat_reports' consensus pass: what one reported alignment contributes to the
// JunctionSet, the DeletionSet and the InsertionSet.  Plain functions over a cigar and a callback: no atomics, no memory of their
// own; thj_juncbed_impl.h runs them on the device, tests/indelsim compiles them for the CPU.
//
//   junctions_from_spliced_hit     junctions.cpp:19-92
//   deletions_from_spliced_hit     deletions.cpp:83-151
//   insertions_from_spliced_hit    insertions.cpp:109-180
//
// Each walker follows its own source: they do not agree on how a dEL moves the genome position (the junction and insertion walkers
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

// the same over a plain cigar array of 16 words (thj_aln: ref_id2 of a fusion alignment in cigar[15])
struct ArrayCigar { const uint32_t* w; THJ_WALK_FN uint32_t operator()(int c) const { return w[c]; } };
template <class F> THJ_WALK_FN int juncs(const uint32_t* cigar, int n_cigar, int32_t left, uint32_t ref_id, F f) { return juncs(n_cigar, left, ref_id, cigar[15], ArrayCigar{cigar}, f); }
template <class F> THJ_WALK_FN int dels(const uint32_t* cigar, int n_cigar, int32_t left, uint32_t ref_id, F f) { return dels(n_cigar, left, ref_id, cigar[15], ArrayCigar{cigar}, f); }
template <class F> THJ_WALK_FN int inss(const uint32_t* cigar, int n_cigar, int32_t left, uint32_t ref_id, F f) { return inss(n_cigar, left, ref_id, cigar[15], ArrayCigar{cigar}, f); }

}  // namespace jbw
