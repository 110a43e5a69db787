// thj_bamsort_core.h -- the order `samtools sort` (0.1.18, by position) gives a BAM file's records:
//
//   bam_sort_core_ext       bam_sort.c:353-414   records are collected until their bytes reach max_mem, every such block is sorted and written
//   bam1_lt                 bam_sort.c:302-308   a block's order: (uint64_t)tid << 32 | (pos + 1), by ks_mergesort (stable, ksort.h:71-118)
//   bam_merge_core          bam_sort.c:202-240   more than one block: a heap over the blocks' head records
//   __pos_cmp, the heap key bam_sort.c:41, :207, :232   (uint64_t)tid << 32 | (uint32_t)(pos + 1) << 1 | strand, then the block, then a counter
//
// A block is sorted without the strand and merged with it, so the merge's inputs are not sorted under its own comparator and the file is
// what the heap gives, not a sort by the merge key.  What it gives has a closed form ("Coordinate-sorted accepted_hits.bam"):
// with more than one block the records come out in the stable order of (tid, pos + 1, tail) over the input order, where tail = 0 for a
// record that stands, among the records of its own (tid, pos) inside its own block, before that block's first reverse-strand record of
// the position, and 1 from that record on; with one block tail = 0 everywhere.  This header holds the two keys with C's integer
// conversions, the block cut and the tail bit, for the kernels of thj_bamsort.hip and for tests/bamsortsim (the CPU build).
#pragma once
#include <stdint.h>

#ifndef THJ_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define THJ_HD __host__ __device__ __forceinline__
#else
#define THJ_HD inline
#endif
#endif

namespace bsort {

enum { FIXED = 32u,            // bam1_core_t as the file holds it: the least a record's block_size can be
       FLAG_REVERSE = 0x10u };

THJ_HD uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// a record behind its block_size field, at any alignment: refID at 4, pos at 8, flag_nc at 16 (FLAG in its high half)
struct Head { uint32_t block_size; int32_t tid, pos; uint32_t strand; };
THJ_HD Head head_of(const uint8_t* rec) {
    Head h;
    h.block_size = rd32(rec); h.tid = (int32_t)rd32(rec + 4); h.pos = (int32_t)rd32(rec + 8);
    h.strand = ((rd32(rec + 16) >> 16) & FLAG_REVERSE) ? 1u : 0u;
    return h;
}
// the record is what its size says: bam_read1 takes block_size + 4 bytes, and 32 of them are the fixed fields
THJ_HD bool head_ok(const Head& h, uint32_t rec_size) { return h.block_size >= FIXED && (uint64_t)h.block_size + 4u == (uint64_t)rec_size; }

// pos + 1 as the int32 the reference adds in (two's complement wrap-around where C leaves it undefined)
THJ_HD int32_t pos1(int32_t pos) { return (int32_t)((uint32_t)pos + 1u); }

// bam1_lt's key: (uint64_t)tid << 32 | (pos + 1).  Both operands are int32 and become uint64_t by sign extension: tid = -1 gives a high
// word of all ones (unmapped records last), pos = -1 a low word of 0, pos < -1 would set every bit
THJ_HD uint64_t block_key(int32_t tid, int32_t pos) { return ((uint64_t)(int64_t)tid << 32) | (uint64_t)(int64_t)pos1(pos); }

// the heap's key: (uint64_t)tid << 32 | (uint32_t)(pos + 1) << 1 | strand -- the shift is a 32-bit one (bit 31 of pos + 1 is lost)
THJ_HD uint64_t merge_key(int32_t tid, int32_t pos, uint32_t strand) {
    return ((uint64_t)(int64_t)tid << 32) | (uint64_t)(uint32_t)((uint32_t)pos1(pos) << 1) | (uint64_t)strand;
}

// the closed form holds where both keys order positions alike: -1 <= pos < 2^31 - 1 (-1 = no position; below it, and where pos + 1
// wraps, the sign extension fills bam1_lt's key with ones and the heap's key does not follow)
THJ_HD bool pos_ok(int32_t pos) { return pos >= -1 && pos < 0x7FFFFFFF; }

// the block cut, a record after the other: mem += rec_size (= 4 + block_size, what bam_read1 returns); a block ends WITH the record
// that brings mem to max_mem, and mem starts again at 0
struct Cut {
    uint64_t mem = 0, max_mem; int64_t ended = 0;
    THJ_HD explicit Cut(uint64_t m) : max_mem(m) {}
    // -> whether the block ends with this record
    THJ_HD bool add(uint32_t rec_size) {
        mem += rec_size;
        if (mem < max_mem) return false;
        mem = 0; ++ended;
        return true;
    }
    // how many blocks the reference writes: one when none ever ended, else the remainder (possibly empty) is one more and all are merged
    THJ_HD int64_t n_blocks() const { return ended ? ended + 1 : 1; }
};

// how many bits of block_key a sort has to look at: 32 and the bits of the largest tid, or all 64 when a tid is negative
THJ_HD int key_bits(bool any_negative_tid, uint32_t max_tid) {
    if (any_negative_tid) return 64;
    int b = 0;
    while (b < 32 && (max_tid >> b)) ++b;
    return 32 + b;
}

// the block of record i: block_start[0 .. n_blocks) rising, block_start[0] = 0 (an empty last block starts at the record count)
THJ_HD uint32_t block_of(const uint32_t* block_start, uint32_t n_blocks, uint32_t i) {
    uint32_t lo = 0, hi = n_blocks;            // the last b with block_start[b] <= i
    while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (block_start[mid] <= i) lo = mid; else hi = mid; }
    return lo;
}

// the tail bit along one block's records of one (tid, pos), in input order: seen = whether a reverse-strand record has come, itself included
THJ_HD uint32_t tail_step(uint32_t& seen, uint32_t strand) { seen |= strand; return seen; }

// where entry i of a key's run [s, e) goes when the run is split stably by the tail bit: z(k) = how many entries before k (of the whole
// sorted list) have tail 0
THJ_HD uint32_t tail_place(uint32_t s, uint32_t e, uint32_t i, uint32_t tail, uint32_t z_s, uint32_t z_i, uint32_t z_e) {
    const uint32_t zeros_before = z_i - z_s;
    return tail ? s + (z_e - z_s) + ((i - s) - zeros_before) : s + zeros_before;
}

}  // namespace bsort
