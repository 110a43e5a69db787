// thj_bamsort.hip -- the context's BAM stream put into the order `samtools sort` (0.1.18, by position) gives the file (thj_bam_stream_sort):
// what tophat.py runs over tophat_reports' part file before it calls the result accepted_hits.bam.  The rule, the closed form the
// device computes and why it holds: thj_bamsort_core.h and DESIGN.md ("Coordinate-sorted accepted_hits.bam").
//
//   (scan)               sizes -> every record's offset in the stream (thj_scan.h; n + 1 entries, so a size is the difference of two)
//   thj_k_bs_keys        a lane per record: block_size, refID, pos and FLAG from the record's bytes at any alignment; 4 + block_size must be
//                        the size and block_size >= 32; bam1_lt's key, and the record's index with its strand in the top bit
//   (radix sort)         hipcub::DeviceRadixSort::SortPairs of (key, index), stable, over the bits in use: 32 and the bits of the largest
//                        refID, all 64 when one is negative
//   more than one block (the reference merges its sorted blocks with a heap whose key also holds the strand):
//   thj_k_bs_flags       in sorted order: where a key's run begins, and where a segment -- one block's records of one key -- begins
//                        (a record's block: bisection of its index in the block starts the host cut from the sizes)
//   (scans)              run and segment numbers
//   thj_k_bs_starts      the runs' starts by number
//   thj_k_bs_firstrev    per segment the first reverse-strand entry (atomicMin): the tail bit of an entry is "not before it" -- the
//                        segmented OR-scan of the strands, said with one minimum per segment
//   thj_k_bs_tail, (scan), thj_k_bs_place    every run split stably by the tail bit: an entry's place from the count of tail-0 entries before it
//   thj_k_bs_sizes       the sizes in the new order; (scan) -> the new offsets
//   thj_k_bs_gather      a WAVE per record in a grid-stride loop: the record's bytes from their old place to their new one through
//                        WaveSink::copy (aligned dword stores, funnel-shifted from the source), into a second buffer of the stream's size
//                        (the context's deflate scratch, grown to it); the two buffers are swapped.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/thj.h"
#include "thj_ctx.h"
#include "thj_scan.h"
#include "thj_bamsort_core.h"
#include "thj_wave_sink.h"

namespace {

typedef unsigned long long u64;
static constexpr uint32_t IDX = 0x7FFFFFFFu;             // a sorted value: the record's index, its strand above it
enum { BS_BAD = 0, BS_MAX_TID = 1, BS_NEG_TID = 2, BS_FIRST_BAD = 3, BS_COUNTERS = 4 };
enum { BAD_SIZE = 1u, BAD_POS = 2u };

__global__ __launch_bounds__(256) void thj_k_bs_keys(const uint8_t* __restrict__ stream, const u64* __restrict__ off, int64_t n, u64* __restrict__ key,
                                                     uint32_t* __restrict__ val, unsigned int* counters) {
    uint32_t bad = 0, max_tid = 0, neg = 0, first_bad = 0xFFFFFFFFu;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const u64 at = off[i];
        const uint32_t size = (uint32_t)(off[i + 1] - at);          // >= 36: the host has looked at the sizes
        const bsort::Head h = bsort::head_of(stream + at);
        uint32_t b = bsort::head_ok(h, size) ? 0u : BAD_SIZE;
        if (!bsort::pos_ok(h.pos)) b |= BAD_POS;
        if (b) { bad |= b; if ((uint32_t)i < first_bad) first_bad = (uint32_t)i; }
        if (h.tid < 0) neg = 1u; else if ((uint32_t)h.tid > max_tid) max_tid = (uint32_t)h.tid;
        key[i] = bsort::block_key(h.tid, h.pos);
        val[i] = (uint32_t)i | (h.strand << 31);
    }
    if (bad) { atomicOr(&counters[BS_BAD], bad); atomicMin(&counters[BS_FIRST_BAD], first_bad); }
    if (max_tid) atomicMax(&counters[BS_MAX_TID], max_tid);
    if (neg) atomicOr(&counters[BS_NEG_TID], 1u);
}

__global__ __launch_bounds__(256) void thj_k_bs_flags(const u64* __restrict__ key, const uint32_t* __restrict__ val, int64_t n, const uint32_t* __restrict__ block_start,
                                                      uint32_t n_blocks, uint32_t* __restrict__ run_head, uint32_t* __restrict__ seg_head) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t rh = i == 0 || key[i] != key[i - 1] ? 1u : 0u;
        run_head[i] = rh;
        seg_head[i] = rh || bsort::block_of(block_start, n_blocks, val[i] & IDX) != bsort::block_of(block_start, n_blocks, val[i - 1] & IDX) ? 1u : 0u;
    }
}
// run[i], seg[i]: the exclusive sums of the head flags on the way in, the entry's run and segment numbers on the way out
__global__ __launch_bounds__(256) void thj_k_bs_starts(const uint32_t* __restrict__ run_head, const uint32_t* __restrict__ seg_head, int64_t n, uint32_t* __restrict__ run,
                                                       uint32_t* __restrict__ seg, uint32_t* __restrict__ run_start) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t r = run[i] + run_head[i] - 1u;
        if (run_head[i]) run_start[r] = (uint32_t)i;
        if (i == n - 1) run_start[r + 1u] = (uint32_t)n;
        run[i] = r;
        seg[i] = seg[i] + seg_head[i] - 1u;
    }
}
__global__ __launch_bounds__(256) void thj_k_bs_firstrev(const uint32_t* __restrict__ val, const uint32_t* __restrict__ seg, int64_t n, uint32_t* first_rev) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        if (val[i] >> 31) atomicMin(&first_rev[seg[i]], (uint32_t)i);
}
// tail0[i] = 1 for an entry before its segment's first reverse-strand one; entry n is 0, so that the sum over n + 1 entries ends with the total
__global__ __launch_bounds__(256) void thj_k_bs_tail(const uint32_t* __restrict__ seg, const uint32_t* __restrict__ first_rev, int64_t n, uint32_t* __restrict__ tail0) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (int64_t)gridDim.x * blockDim.x)
        tail0[i] = i < n && (uint32_t)i < first_rev[seg[i]] ? 1u : 0u;
}
__global__ __launch_bounds__(256) void thj_k_bs_place(const uint32_t* __restrict__ val, const uint32_t* __restrict__ run, const uint32_t* __restrict__ run_start,
                                                      const uint32_t* __restrict__ tail0, const uint32_t* __restrict__ z, int64_t n, uint32_t* __restrict__ perm) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t r = run[i], s = run_start[r], e = run_start[r + 1u];
        perm[bsort::tail_place(s, e, (uint32_t)i, tail0[i] ^ 1u, z[s], z[i], z[e])] = val[i] & IDX;
    }
}
__global__ __launch_bounds__(256) void thj_k_bs_sizes(const uint32_t* __restrict__ perm, const u64* __restrict__ off, int64_t n, uint32_t* __restrict__ size) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t p = perm[j] & IDX;
        size[j] = (uint32_t)(off[p + 1u] - off[p]);
    }
}
// a wave per record, grid-stride (a short record does not cost a launch slot); the next record's places are asked for before this one is copied
__global__ __launch_bounds__(256) void thj_k_bs_gather(const uint8_t* __restrict__ src, const u64* __restrict__ src_off, const uint32_t* __restrict__ perm,
                                                       const uint32_t* __restrict__ size, const u64* __restrict__ dst_off, int64_t n, uint8_t* out) {
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    int64_t j = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (j >= n) return;
    u64 from = src_off[perm[j] & IDX], to = dst_off[j];
    uint32_t len = size[j];
    while (true) {
        const int64_t next = j + waves;
        u64 from2 = 0, to2 = 0; uint32_t len2 = 0;
        if (next < n) { from2 = src_off[perm[next] & IDX]; to2 = dst_off[next]; len2 = size[next]; }
        WaveSink sink{out + to, lane};
        sink.copy(0u, src + from, len);
        if (next >= n) break;
        j = next; from = from2; to = to2; len = len2;
    }
}

dim3 bs_grid(int64_t n) { const int64_t b = (n + 255) / 256; return dim3((unsigned)(b > 2048 ? 2048 : b < 1 ? 1 : b)); }

}  // namespace

extern "C" int thj_bam_stream_sort(thj_ctx* c, uint32_t* rec_size, int64_t n_records, int64_t max_mem, int64_t* n_blocks) {
    if (!c || n_records < 0 || (n_records > 0 && !rec_size) || max_mem < 1 || !n_blocks) { thj_set_error("thj_bam_stream_sort: bad argument"); return THJ_EINVAL; }
    *n_blocks = 1;
    const int64_t n = n_records;
    if (n >= 0x7FFFFFF0ll) { thj_set_error("thj_bam_stream_sort: more than 2^31 - 17 records"); return THJ_EINVAL; }
    // the sizes against the stream, and the reference's block cut (bam_sort_core_ext), before the device reads a byte
    bsort::Cut cut((uint64_t)max_mem);
    std::vector<uint32_t> block_start{0u};
    uint64_t sum = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (rec_size[i] < 4u + bsort::FIXED) { thj_set_error("thj_bam_stream_sort: record %lld has a size of %u bytes (a record is its block_size field and at least 32 bytes)", (long long)i, rec_size[i]); return THJ_EINVAL; }
        sum += rec_size[i];
        if (cut.add(rec_size[i])) block_start.push_back((uint32_t)(i + 1));
    }
    if (sum != (uint64_t)c->bam_bytes) {
        thj_set_error("thj_bam_stream_sort: the sizes of the %lld records add up to %llu bytes, the stream holds %lld", (long long)n, (unsigned long long)sum, (long long)c->bam_bytes);
        return THJ_EINVAL;
    }
    if (n == 0) return THJ_OK;
    const uint32_t nb = (uint32_t)cut.n_blocks();
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    hipStream_t st = c->stream;
    // 32 bytes a record: two key and two value buffers (what the radix sort reads and writes; the tail pass and the new sizes and offsets
    // live in whichever of them is dead) and the records' offsets.  Every array has room for n + 2 entries
    const size_t m = (size_t)n + 2;
    std::vector<uint32_t> h_size((size_t)n);
    DevTemps tmp;
    u64 *k0, *k1, *off; uint32_t *v0, *v1, *d_bs; void* scratch; unsigned int* counters;
    HIPCHK(tmp.alloc(k0, m * 8)); HIPCHK(tmp.alloc(k1, m * 8)); HIPCHK(tmp.alloc(off, m * 8));
    HIPCHK(tmp.alloc(v0, m * 4)); HIPCHK(tmp.alloc(v1, m * 4));
    HIPCHK(tmp.alloc(scratch, thj_scan::scratch_bytes(n + 1, 8)));
    HIPCHK(tmp.alloc(counters, BS_COUNTERS * 4));
    HIPCHK(tmp.alloc(d_bs, (size_t)nb * 4 + 4));
    const dim3 grid = bs_grid(n);
    // offsets (sizes in v1, a 0 behind them: off[n] = the stream's bytes)
    HIPCHK(hipMemcpyAsync(v1, rec_size, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(v1 + n, 0, 4, st));
    thj_scan::exclusive_sum<uint32_t, u64>(st, (const uint32_t*)v1, off, n + 1, scratch);
    const unsigned int init[BS_COUNTERS] = {0u, 0u, 0u, 0xFFFFFFFFu};
    HIPCHK(hipMemcpyAsync(counters, init, sizeof init, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(thj_k_bs_keys, grid, dim3(256), 0, st, (const uint8_t*)c->d_bam, (const u64*)off, n, k0, v0, counters);
    HIPCHK(hipGetLastError());
    unsigned int h_cnt[BS_COUNTERS];
    HIPCHK(hipMemcpyAsync(h_cnt, counters, sizeof h_cnt, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h_cnt[BS_BAD] & BAD_SIZE) {
        thj_set_error("thj_bam_stream_sort: record %u does not fill its size: 4 + block_size must be the %u bytes given for it, and block_size at least 32", h_cnt[BS_FIRST_BAD], rec_size[h_cnt[BS_FIRST_BAD]]);
        return THJ_EINVAL;
    }
    if (h_cnt[BS_BAD] & BAD_POS) { thj_set_error("thj_bam_stream_sort: record %u has a position below -1 or of 2^31 - 1 (the reference's two keys order such positions differently)", h_cnt[BS_FIRST_BAD]); return THJ_EINVAL; }
    const int bits = bsort::key_bits(h_cnt[BS_NEG_TID] != 0, h_cnt[BS_MAX_TID]);
    if (const int rc = run_with_sort_tmp(c, [&](void* t, size_t& bytes) { return hipcub::DeviceRadixSort::SortPairs(t, bytes, (const u64*)k0, k1, (const uint32_t*)v0, v1, (int)n, 0, bits, st); })) return rc;
    const uint32_t* perm = v1;           // one block: the sorted indices are the order
    uint32_t* d_size = v0; u64* d_off = k0;
    if (nb > 1) {
        uint32_t *f0 = (uint32_t*)k0, *f1 = (uint32_t*)k0 + m, *f2 = v0, *f3 = (uint32_t*)k1, *f4 = (uint32_t*)k1 + m;
        HIPCHK(hipMemcpyAsync(d_bs, block_start.data(), (size_t)block_start.size() * 4, hipMemcpyHostToDevice, st));
        // (the cut may have ended with the last record: the empty block behind it holds no record and is never looked up)
        hipLaunchKernelGGL(thj_k_bs_flags, grid, dim3(256), 0, st, (const u64*)k1, (const uint32_t*)v1, n, (const uint32_t*)d_bs, (uint32_t)block_start.size(), f0, f1);
        HIPCHK(hipGetLastError());
        thj_scan::exclusive_sum<uint32_t, uint32_t>(st, (const uint32_t*)f0, f3, n, scratch);           // (the sorted keys are dead from here)
        thj_scan::exclusive_sum<uint32_t, uint32_t>(st, (const uint32_t*)f1, f4, n, scratch);
        hipLaunchKernelGGL(thj_k_bs_starts, grid, dim3(256), 0, st, (const uint32_t*)f0, (const uint32_t*)f1, n, f3, f4, f2);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemsetAsync(f0, 0xFF, (size_t)n * 4, st));
        hipLaunchKernelGGL(thj_k_bs_firstrev, grid, dim3(256), 0, st, (const uint32_t*)v1, (const uint32_t*)f4, n, f0);
        hipLaunchKernelGGL(thj_k_bs_tail, grid, dim3(256), 0, st, (const uint32_t*)f4, (const uint32_t*)f0, n, f1);
        HIPCHK(hipGetLastError());
        thj_scan::exclusive_sum<uint32_t, uint32_t>(st, (const uint32_t*)f1, f4, n + 1, scratch);       // z, over the segment numbers
        hipLaunchKernelGGL(thj_k_bs_place, grid, dim3(256), 0, st, (const uint32_t*)v1, (const uint32_t*)f3, (const uint32_t*)f2, (const uint32_t*)f1, (const uint32_t*)f4, n, f0);
        HIPCHK(hipGetLastError());
        perm = f0; d_off = k1;
    }
    hipLaunchKernelGGL(thj_k_bs_sizes, grid, dim3(256), 0, st, perm, (const u64*)off, n, d_size);
    HIPCHK(hipGetLastError());
    thj_scan::exclusive_sum<uint32_t, u64>(st, (const uint32_t*)d_size, d_off, n, scratch);
    HIPCHK(hipMemcpyAsync(h_size.data(), d_size, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    // the second buffer: the deflater's scratch, grown to the stream (thj_bgzf_deflate sizes it again for itself)
    const size_t need = (size_t)c->bam_bytes + 64;
    if (c->bam_tmp_cap < need) {
        HIPCHK(hipStreamSynchronize(st));
        if (c->d_bam_tmp) (void)hipFree(c->d_bam_tmp);
        c->d_bam_tmp = nullptr; c->bam_tmp_cap = 0;
        HIPCHK(hipMalloc(&c->d_bam_tmp, need));
        c->bam_tmp_cap = need;
    }
    const int64_t gw = (n + 3) / 4;
    hipLaunchKernelGGL(thj_k_bs_gather, dim3((unsigned)(gw > 2048 ? 2048 : gw)), dim3(256), 0, st, (const uint8_t*)c->d_bam, (const u64*)off, perm, (const uint32_t*)d_size,
                       (const u64*)d_off, n, (uint8_t*)c->d_bam_tmp);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    uint8_t* sorted = (uint8_t*)c->d_bam_tmp; const size_t sorted_cap = c->bam_tmp_cap;
    c->d_bam_tmp = c->d_bam; c->bam_tmp_cap = c->bam_cap;
    c->d_bam = sorted; c->bam_cap = sorted_cap;
    memcpy(rec_size, h_size.data(), (size_t)n * 4);
    *n_blocks = (int64_t)nb;
    return THJ_OK;
}
