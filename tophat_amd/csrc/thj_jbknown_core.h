// thj_jbknown_core.h -- the two inputs of tophat_reports' consensus that are decided per record and per distinct junction:
//
//   the read filter        read_best_alignments / exclude_hits_on_filtered_junctions   tophat_reports.cpp:133-136, :1202-1205
//   the annotated junctions (--gtf-juncs) in filter_junctions / knockout_shadow_junctions   junctions.cpp:270, :305-318
//
// Plain functions without memory of their own: thj_juncbed_impl.h runs them in its kernels, thj_reported_core.h and thj_junctions'
// host reader fill thj_aln.mismatches with them, tests/jbknownsim compiles them for the CPU.
//
// The three quantities of the filter, as the reference's BAM factory makes them (BAMHitFactory::get_hit_from_buf):
//   mismatches   unsigned char num_mismatches = NM (bam_aux2i cut to 8 bits; no NM: 0), then "-= length" for every INS and every DEL
//                of the cigar it builds, modulo 256 (bwt_map.cpp:1175-1188, :1362-1365): an indel record without NM has 256 - length
//                mismatches and no limit lets it through.  Only the UPPER-case ops are subtracted.  A fusion alignment is rebuilt
//                from XF:Z and the subtraction runs over THAT cigar (:1282-1285), again INS and DEL only: the iNS / dEL of a piece
//                that runs down the genome stay in the count, while the record's own CIGAR column (one of the two pieces) is never
//                looked at.
//   gap_length   the lengths of INS, iNS, DEL and dEL (bwt_map.cpp:32-43)
//   edit_dist    num_mismatches + gap_length, kept in an unsigned char (:1429-1430)
// thj_aln.mismatches holds the first; the other two come from it and the cigar.  (thj_aln.edit_dist is something else: NM itself,
// clamped, which the fusion set reads.)
#pragma once
#include <stdint.h>
#include "thj_jb_walk.h"

#ifndef THJ_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define THJ_HD __host__ __device__ __forceinline__
#else
#define THJ_HD inline
#endif
#endif

namespace jbk {

// ---- the read filter

struct ReadFilter { int32_t on, read_mismatches, read_gap_length, read_edit_dist; };

template <class CG>
THJ_HD uint32_t gap_length(int n_cigar, CG cg) {
    uint32_t g = 0;
    for (int c = 0; c < n_cigar; ++c) { const uint32_t op = cg(c) >> 28; if (op >= 3u && op <= 6u) g += cg(c) & jbw::LEN_MASK; }
    return g;
}

// thj_aln.mismatches of a record whose NM tag reads nm (absent: 0) and whose cigar -- the one the alignment is rebuilt with -- is cg
template <class CG>
THJ_HD uint8_t mismatches(int64_t nm, int n_cigar, CG cg) {
    uint32_t v = (uint32_t)(uint8_t)nm;
    for (int c = 0; c < n_cigar; ++c) { const uint32_t op = cg(c) >> 28; if (op == 3u || op == 5u) v -= cg(c) & jbw::LEN_MASK; }
    return (uint8_t)v;
}

// does the filter drop the record?  It is then gone for every set and both passes.
template <class CG>
THJ_HD bool dropped(const ReadFilter& f, uint32_t mism, int n_cigar, CG cg) {
    const uint32_t gap = gap_length(n_cigar, cg);
    const int32_t ed = (int32_t)(uint8_t)(mism + gap);
    return (int32_t)mism > f.read_mismatches || (int64_t)gap > (int64_t)f.read_gap_length || ed > f.read_edit_dist;
}

// ---- the annotated junctions.  Keys are junc_key's (thj_core.h): [global left + 1 : 34 | right - left : 29 | antisense : 1].

typedef unsigned long long key64;                               // (thj::u64)
static constexpr key64 SPAN_MASK = (1ull << 29) - 1;

// Can an entry of the annotation equal a junction of a record?  Not on a contig the genome does not hold, and not with a span
// outside 1 .. 2^29 - 1 or a left end outside its contig (-1 .. length - 1): junc_key would fold such an entry onto some other
// junction's key, so it is dropped before it is packed.
THJ_HD bool known_entry_ok(uint32_t ref_id, uint32_t left, uint32_t right, int32_t n_contigs, const int64_t* contig_len) {
    if (ref_id < 1u || (int64_t)ref_id > (int64_t)n_contigs) return false;
    const uint32_t span = right - left;
    if (span < 1u || span > (uint32_t)SPAN_MASK) return false;
    const int64_t l = (int64_t)(int32_t)left;
    return l >= -1 && l < contig_len[ref_id - 1];
}

// gtf_junctions.find(junction) over the sorted, unique keys
THJ_HD bool known(const key64* keys, int64_t n, key64 k) {
    int64_t a = 0, b = n;
    while (a < b) { const int64_t m = (a + b) >> 1; if (keys[m] < k) a = m + 1; else b = m; }
    return a < n && keys[a] == k;
}

// what filter_junctions' loop leaves in a junction's `accepted` (and `gtf_match`): the values of the consensus table's acc column
enum : uint32_t { ACC_REJECTED = 0, ACC_VALID = 1, ACC_KNOWN = 2 };

// junctions.cpp:305-315: a junction of the annotation is accepted whatever its extents, length and support; any other goes through
// accept_if_valid (:192-240; no splice mismatches are recorded).  keys == nullptr: no annotation.
THJ_HD uint32_t accept(key64 key, uint32_t left_extent, uint32_t right_extent, uint32_t support, int min_anchor, const key64* keys, int64_t n_keys) {
    if (keys && known(keys, n_keys, key)) return ACC_KNOWN;
    const uint32_t mn = left_extent < right_extent ? left_extent : right_extent, len = (uint32_t)((key >> 1) & SPAN_MASK);
    if ((int)mn < min_anchor) return ACC_REJECTED;
    if (len > 50000u) return support >= 2u && mn > 12u ? ACC_VALID : ACC_REJECTED;
    return ACC_VALID;
}

// knockout_shadow_junctions looks for stronger neighbours of "accepted && !gtf_match" junctions only (junctions.cpp:270)
THJ_HD bool accepted(uint32_t acc) { return acc != ACC_REJECTED; }
THJ_HD bool exempt(uint32_t acc) { return acc == ACC_KNOWN; }

}  // namespace jbk
