// thj_juncbed_impl.h -- junction consensus of tophat_reports on the device: the alignments
// long_spanning_reads left resident in HBM (or any records handed in) reduced to the JunctionSet that junctions.bed prints.
//
//   junctions_from_spliced_hit / junctions_from_alignment / JunctionStats::merge_with   junctions.cpp:19-142, junctions.h:87-101
//   accept_if_valid, knockout_shadow_junctions (filter_junctions)                        junctions.cpp:192-330
//   exclude_hits_on_filtered_junctions + update_junctions of the second pass             tophat_reports.cpp:1182-1230
//   the final extent filter                                                              tophat_reports.cpp:2974-2984
//
// A segmented reduce in hash-table form.  Pass 1: every REF_SKIP of every record is one "occurrence"; its junction key goes
// into an open-addressing table (support += 1, extents = max) and the occurrence is kept -- 16 bytes: table slot, extents,
// position inside its record -- because the second pass needs it again after the filter.  Filter: accept_if_valid per
// distinct junction; the distinct keys are radix-sorted and every accepted junction looks at its opposite-strand neighbours
// within min_anchor_len.  Pass 2: a record all of whose junctions survived adds its occurrences to the final statistics.
// All integer work; the order in which records arrive does not matter (sums and maxima).
// On request the same two passes give the InsertionSet and the DeletionSet (insertions.bed, deletions.bed): thj_juncbed_indel_impl.h;
// there the order of the records does matter for one thing, the letters an insertion is printed with.  And the FusionSet
// (fusions.out): thj_juncbed_fusion_impl.h.
//
// Included at the end of thj_span.hip.  Not part of the timed hot path of bench.py unless asked for.
#pragma once
#include <tuple>
#include "thj_jb_walk.h"

struct JbOcc { uint32_t slot; uint16_t le, re; uint8_t nj, idx; uint16_t pad; uint32_t pad2; };      // 16 bytes
static_assert(sizeof(JbOcc) == 16, "occurrence layout");

struct JbTable {
    u64* key; u64 mask;
    uint32_t *cnt1, *le1, *re1, *cnt2, *le2, *re2, *left, *acc;
    u64* list;                         // distinct keys in arrival order
    unsigned long long* counters;      // [0] distinct, [1] occurrences counted, [2] occurrences written, [3] overflow flag,
                                       // [4] indel occurrences counted, [5] written, [6] JBI_FLAG_* (thj_juncbed_indel_impl.h)
};

__device__ __forceinline__ u64 jb_mix(u64 x) { x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull; x ^= x >> 27; x *= 0x94d049bb133111ebull; x ^= x >> 31; return x; }

__device__ __forceinline__ uint32_t jb_insert(const JbTable& t, u64 k, uint32_t left) {
    u64 h = jb_mix(k) & t.mask;
    for (u64 probe = 0; probe <= t.mask; ++probe) {
        u64 cur = __hip_atomic_load(&t.key[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == ~0ull) {
            const u64 old = atomicCAS((unsigned long long*)&t.key[h], ~0ull, k);
            if (old == ~0ull) { const unsigned long long pos = atomicAdd(&t.counters[0], 1ull); if (pos <= t.mask) t.list[pos] = k; t.left[h] = left; cur = k; }
            else cur = old;
        }
        if (cur == k) return (uint32_t)h;
        h = (h + 1) & t.mask;
    }
    atomicExch(&t.counters[3], 1ull);
    return 0xFFFFFFFFu;
}

// the junctions of one record (junctions_from_spliced_hit, junctions.cpp:19-92; the walk itself: jbw::juncs, thj_jb_walk.h): calls
// f(ref_id, left, right, left_extent, right_extent) per REF_SKIP / rEF_SKIP.
// slot: the record is in the stitch kernels' slot layout (RecSink, thj_span.hip: cigar ops 4.. live in the tail line)
struct JbCigar { const uint32_t* w; bool slot; __device__ __forceinline__ uint32_t operator()(int c) const { return w[slot && c >= 4 ? 12 + c : 6 + c]; } };
template <class F>
__device__ __forceinline__ int jb_rec_juncs(const OutAln& a, bool slot, F f) {
    const JbCigar cg{(const uint32_t*)&a, slot};
    return jbw::juncs(a.n_cigar < SPAN_MAXC ? a.n_cigar : SPAN_MAXC, a.left, a.ref_id, cg(SPAN_MAXC - 1), cg, f);
}

// record i of a pass: slots (first record of every read that has one) then the extra pool; or a plain array
struct JbRecs { const OutAln* slots; const uint8_t* nrec; int64_t n_slots; const OutAln* extra; int64_t n_extra; bool slot_layout; };
__device__ __forceinline__ const OutAln* jb_rec(const JbRecs& r, int64_t i) {
    if (i < r.n_slots) return (!r.nrec || r.nrec[i]) ? &r.slots[i] : nullptr;
    return &r.extra[i - r.n_slots];
}

#include "thj_juncbed_indel_impl.h"

// INDEL: the records' DEL / dEL / INS / iNS ops are counted too (counters[4]; plain arrays only)
template <bool INDEL>
__global__ __launch_bounds__(256) void thj_k_jb_count(JbRecs r, unsigned long long* counters) {
    __shared__ unsigned int s_n, s_i;
    if (threadIdx.x == 0) { s_n = 0; s_i = 0; }
    __syncthreads();
    unsigned int mine = 0, mine_i = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < r.n_slots + r.n_extra; i += (int64_t)gridDim.x * blockDim.x) {
        const OutAln* a = jb_rec(r, i);
        if (a) mine += (unsigned)jb_rec_juncs(*a, r.slot_layout, [](uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) {});
        if (INDEL && a) mine_i += (unsigned)jbi_rec_count(*a);
    }
    if (mine) atomicAdd(&s_n, mine);
    if (INDEL && mine_i) atomicAdd(&s_i, mine_i);
    __syncthreads();
    if (threadIdx.x == 0 && s_n) atomicAdd(&counters[1], (unsigned long long)s_n);
    if (INDEL && threadIdx.x == 0 && s_i) atomicAdd(&counters[4], (unsigned long long)s_i);
}

// one reservation per wave: inclusive scan of n over the lanes, the last lane adds the total; returns where this lane's share starts
__device__ __forceinline__ unsigned long long jb_wave_reserve(unsigned long long* counter, unsigned int n, int lane) {
    unsigned int incl = n;
    for (int d = 1; d < 64; d <<= 1) { const unsigned int up = __shfl_up(incl, d); if (lane >= d) incl += up; }
    const unsigned int wave_total = __shfl(incl, 63);
    unsigned long long base = 0;
    if (lane == 63 && wave_total) base = atomicAdd(counter, (unsigned long long)wave_total);
    base = __shfl(base, 63);
    return base + incl - n;
}

// INDEL: beside the junction occurrences the records' indel occurrences are listed (iocc; record i of this call has ordinal ord_base + i)
template <bool INDEL>
__global__ __launch_bounds__(256) void thj_k_jb_add(Genome g, JbRecs r, JbTable t, JbOcc* occ, unsigned long long occ_cap,
                                                    JbiSeq sq, JbiOcc* iocc, unsigned long long iocc_cap, u64 ord_base) {
    const int lane = threadIdx.x & 63;
    const int64_t total = r.n_slots + r.n_extra;
    // whole waves walk together so that the wave-wide reservations below see every lane
    const int64_t n_iter = (total + (int64_t)gridDim.x * blockDim.x - 1) / ((int64_t)gridDim.x * blockDim.x);
    for (int64_t it = 0; it < n_iter; ++it) {
        const int64_t i = it * (int64_t)gridDim.x * blockDim.x + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        const OutAln* a = i < total ? jb_rec(r, i) : nullptr;
        unsigned int nj = a ? (unsigned)jb_rec_juncs(*a, r.slot_layout, [](uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) {}) : 0u;
        const unsigned long long first = jb_wave_reserve(&t.counters[2], nj, lane);
        if (nj) {
            unsigned long long at = first;
            const bool anti = (a->flags & 4u) != 0;             // THJ_HIT_ANTISENSE_SPLICE
            uint8_t idx = 0;
            const uint8_t n8 = (uint8_t)nj;
            jb_rec_juncs(*a, r.slot_layout, [&](uint32_t ref, uint32_t left, uint32_t right, uint32_t le, uint32_t re) {
                const uint32_t slot = jb_insert(t, junc_key(g, ref, left, right, anti), left);
                if (slot != 0xFFFFFFFFu) {
                    atomicAdd(&t.cnt1[slot], 1u);
                    atomicMax(&t.le1[slot], le);
                    atomicMax(&t.re1[slot], re);
                }
                if (at < occ_cap) occ[at] = JbOcc{slot, (uint16_t)(le > 65535u ? 65535u : le), (uint16_t)(re > 65535u ? 65535u : re), n8, idx, 0, 0};
                ++at; ++idx;
            });
        }
        if (INDEL) {
            const unsigned int ni = a ? (unsigned)jbi_rec_count(*a) : 0u;
            const unsigned long long iat = jb_wave_reserve(&t.counters[5], ni, lane);
            if (ni) jbi_rec_write(g, *a, i, ord_base + (u64)i, nj ? (u64)first : JBI_NO_JUNC, sq, iocc, iat, iocc_cap, &t.counters[6]);
        }
    }
}

// accept_if_valid (junctions.cpp:192-242) per distinct junction
__global__ __launch_bounds__(256) void thj_k_jb_accept(JbTable t, int64_t n, int min_anchor) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= (int64_t)t.mask; i += (int64_t)gridDim.x * blockDim.x) {
        const u64 k = t.key[i];
        if (k == ~0ull) continue;
        const uint32_t le = t.le1[i], re = t.re1[i], mn = le < re ? le : re, len = (uint32_t)((k >> 1) & ((1ull << 29) - 1));
        uint32_t ok;
        if ((int)mn < min_anchor) ok = 0;
        else if (len > 50000u) ok = t.cnt1[i] >= 2u && mn > 12u;
        else ok = 1;
        t.acc[i] = ok;
    }
    (void)n;
}

__device__ __forceinline__ uint32_t jb_find(const JbTable& t, u64 k) {
    u64 h = jb_mix(k) & t.mask;
    for (u64 probe = 0; probe <= t.mask; ++probe) {
        const u64 cur = t.key[h];
        if (cur == k) return (uint32_t)h;
        if (cur == ~0ull) return 0xFFFFFFFFu;
        h = (h + 1) & t.mask;
    }
    return 0xFFFFFFFFu;
}

// knockout_shadow_junctions (junctions.cpp:244-315) over the sorted distinct keys: an accepted junction loses to a junction of
// the other strand that starts within min_anchor_len before it (or at it, ending within min_anchor_len after it) when that
// one has more support.  Writes acc2 (the junction's own flag only, as the reference does).
__global__ __launch_bounds__(256) void thj_k_jb_knockout(JbTable t, const u64* sorted, int64_t n, int min_anchor, uint32_t* acc2) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const u64 k = sorted[i];
        const uint32_t si = jb_find(t, k);
        uint32_t ok = t.acc[si];
        if (ok && t.left[si] >= (uint32_t)min_anchor) {        // left < anchor: the reference's unsigned left wraps, the range is empty
            const u64 anti = k & 1ull, len = (k >> 1) & ((1ull << 29) - 1), gp = k >> 30;
            // fuzzy_left = (left - anchor, right, !strand), fuzzy_right = (left, right + anchor, !strand): in (left, right - left)
            // key space both have the length field len + anchor
            const u64 len2 = (len + (u64)min_anchor) & ((1ull << 29) - 1);
            const u64 lo = ((gp - (u64)min_anchor) << 30) | (len2 << 1) | (anti ^ 1ull);
            const u64 hi = (gp << 30) | (len2 << 1) | (anti ^ 1ull);
            int64_t a = 0, b = n;                              // lower_bound(lo)
            while (a < b) { const int64_t m = (a + b) >> 1; if (sorted[m] < lo) a = m + 1; else b = m; }
            const uint32_t my_support = t.cnt1[si];
            for (int64_t q = a; q < n && sorted[q] <= hi; ++q) {
                const u64 k2 = sorted[q];
                if (q == i || (k2 & 1ull) == anti) continue;
                const int64_t left_diff = (int64_t)gp - (int64_t)(k2 >> 30);
                const int64_t right_diff = ((int64_t)gp + (int64_t)len) - ((int64_t)(k2 >> 30) + (int64_t)((k2 >> 1) & ((1ull << 29) - 1)));
                if (left_diff < min_anchor || right_diff < min_anchor) {
                    const uint32_t s2 = jb_find(t, k2);
                    if (my_support < t.cnt1[s2]) ok = 0;
                }
            }
        }
        acc2[si] = ok;
    }
}

// second pass: the first occurrence of a record speaks for the record
__global__ __launch_bounds__(256) void thj_k_jb_second(JbTable t, const JbOcc* occ, int64_t n_occ, const uint32_t* acc2) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_occ; i += (int64_t)gridDim.x * blockDim.x) {
        const JbOcc o = occ[i];
        if (o.idx != 0) continue;
        bool ok = true;
        for (int k = 0; k < o.nj; ++k) { const uint32_t s = occ[i + k].slot; if (s == 0xFFFFFFFFu || !acc2[s]) ok = false; }
        if (!ok) continue;
        for (int k = 0; k < o.nj; ++k) {
            const JbOcc q = occ[i + k];
            atomicAdd(&t.cnt2[q.slot], 1u);
            atomicMax(&t.le2[q.slot], (uint32_t)q.le);
            atomicMax(&t.re2[q.slot], (uint32_t)q.re);
        }
    }
}

struct JbOut { u64 key; uint32_t support, le, re, left; };
__global__ __launch_bounds__(256) void thj_k_jb_gather(JbTable t, const u64* sorted, int64_t n, JbOut* out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t s = jb_find(t, sorted[i]);
        out[i] = JbOut{sorted[i], t.cnt2[s], t.le2[s], t.re2[s], t.left[s]};
    }
}

#include "thj_juncbed_fusion_impl.h"

// ------------------------------------------------------------------------------------------------ host side

static void jb_free(thj_ctx* c) {
    hipFree(c->d_jb_key); hipFree(c->d_jb_u32); hipFree(c->d_jb_list); hipFree(c->d_jb_cnt); hipFree(c->d_jb_occ); hipFree(c->d_jb_sorted);
    c->d_jb_key = nullptr; c->d_jb_u32 = nullptr; c->d_jb_list = nullptr; c->d_jb_cnt = nullptr; c->d_jb_occ = nullptr; c->d_jb_sorted = nullptr;
    c->jb_cap = 0; c->jb_occ_cap = 0;
    hipFree(c->d_jbi_u64); hipFree(c->d_jbi_u32); hipFree(c->d_jbi_cnt); hipFree(c->d_jbi_occ);
    c->d_jbi_u64 = nullptr; c->d_jbi_u32 = nullptr; c->d_jbi_cnt = nullptr; c->d_jbi_occ = nullptr;
    c->jbi_cap = 0; c->jbi_occ_cap = 0; c->jbi_on = false;
    hipFree(c->d_jbf_u64); hipFree(c->d_jbf_u32); hipFree(c->d_jbf_cnt); hipFree(c->d_jbf_grp); hipFree(c->d_jbf_focc); hipFree(c->d_jbf_uocc); hipFree(c->d_jbf_jocc);
    c->d_jbf_u64 = nullptr; c->d_jbf_u32 = nullptr; c->d_jbf_cnt = nullptr; c->d_jbf_grp = nullptr; c->d_jbf_focc = nullptr; c->d_jbf_uocc = nullptr; c->d_jbf_jocc = nullptr;
    c->jbf_cap = 0; c->jbf_groups = 0; c->jbf_groups_cap = 0; c->jbf_focc_cap = 0; c->jbf_uocc_cap = 0; c->jbf_jocc_cap = 0; c->jbf_on = false;
}

static JbTable jb_table(thj_ctx* c) {
    uint32_t* u = c->d_jb_u32; const int64_t n = c->jb_cap;
    return JbTable{c->d_jb_key, (u64)n - 1, u, u + n, u + 2 * n, u + 3 * n, u + 4 * n, u + 5 * n, u + 6 * n, u + 7 * n, c->d_jb_list, c->d_jb_cnt};
}
// which: 0 the deletion table, 1 the insertion table (only that one has priorities and letters)
static JbiTable jbi_table(thj_ctx* c, int which) {
    const int64_t n = c->jbi_cap;
    u64* u = c->d_jbi_u64 + (size_t)which * 4 * n; uint32_t* w = c->d_jbi_u32 + (size_t)which * 3 * n;
    return JbiTable{u, which ? u + n : nullptr, which ? u + 2 * n : nullptr, u + 3 * n, (u64)n - 1, w, w + n, w + 2 * n, &c->d_jbi_cnt[which], &c->d_jbi_cnt[2]};
}

static int jb_alloc(thj_ctx* c, int64_t cap) {
    int64_t p = 1 << 16;
    while (p < cap) p <<= 1;
    if (p == c->jb_cap) return THJ_OK;
    hipFree(c->d_jb_key); hipFree(c->d_jb_u32); hipFree(c->d_jb_list); hipFree(c->d_jb_sorted);
    c->d_jb_key = nullptr; c->d_jb_u32 = nullptr; c->d_jb_list = nullptr; c->d_jb_sorted = nullptr; c->jb_cap = 0;
    HIPCHK(hipMalloc(&c->d_jb_key, (size_t)p * 8));
    HIPCHK(hipMalloc(&c->d_jb_u32, (size_t)p * 4 * 9));        // cnt1 le1 re1 cnt2 le2 re2 left acc acc2
    HIPCHK(hipMalloc(&c->d_jb_list, (size_t)p * 8));
    HIPCHK(hipMalloc(&c->d_jb_sorted, (size_t)p * 8));
    if (!c->d_jb_cnt) HIPCHK(hipMalloc(&c->d_jb_cnt, 8 * sizeof(unsigned long long)));
    c->jb_cap = p;
    return THJ_OK;
}
// the two indel tables: as many slots each as the junction table has
static int jbi_alloc(thj_ctx* c) {
    if (c->jbi_cap == c->jb_cap && c->d_jbi_u64) return THJ_OK;
    hipFree(c->d_jbi_u64); hipFree(c->d_jbi_u32);
    c->d_jbi_u64 = nullptr; c->d_jbi_u32 = nullptr; c->jbi_cap = 0;
    HIPCHK(hipMalloc(&c->d_jbi_u64, (size_t)c->jb_cap * 8 * 8));     // per table: key prio bases list
    HIPCHK(hipMalloc(&c->d_jbi_u32, (size_t)c->jb_cap * 4 * 6));     // per table: support, left extent, right extent
    if (!c->d_jbi_cnt) HIPCHK(hipMalloc(&c->d_jbi_cnt, 4 * sizeof(unsigned long long)));
    c->jbi_cap = c->jb_cap;
    return THJ_OK;
}

extern "C" int thj_juncbed_configure(thj_ctx* c, int64_t junction_capacity) {
    if (!c || junction_capacity < 1) { thj_set_error("thj_juncbed_configure: bad argument"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->jb_want = junction_capacity;
    return THJ_OK;
}

extern "C" int thj_juncbed_reset_async(thj_ctx* c) {
    if (!c) { thj_set_error("null ctx"); return THJ_EINVAL; }
    if (!c->d_blocks) { thj_set_error("no genome resident: call thj_genome_upload/adopt first"); return THJ_ESTATE; }
    HIPCHK(hipSetDevice(c->device));
    // twice the candidate set long_spanning_reads was given (its records cannot hold other junctions than those and the ones
    // already in spliced segment hits), at least 2^20 slots, or what thj_juncbed_configure asked for
    int64_t want = c->jb_want > 0 ? c->jb_want : (c->n_span_junc * 4 > (1 << 20) ? c->n_span_junc * 4 : (1 << 20));
    HIPCHK(hipStreamSynchronize(c->stream));
    int rc = jb_alloc(c, want);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(c->d_jb_key, 0xFF, (size_t)c->jb_cap * 8, c->stream));
    HIPCHK(hipMemsetAsync(c->d_jb_u32, 0, (size_t)c->jb_cap * 4 * 9, c->stream));
    HIPCHK(hipMemsetAsync(c->d_jb_cnt, 0, 8 * sizeof(unsigned long long), c->stream));
    c->jb_occ_used = 0;
    c->h_jb.clear();
    c->jbi_on = false; c->jbi_occ_used = 0; c->jb_records = 0;
    c->h_jbi_ins.clear(); c->h_jbi_del.clear();
    c->jbf_on = false; c->jbf_groups = 0; c->h_jbf.clear();
    return THJ_OK;
}

extern "C" int thj_juncbed_collect_indels(thj_ctx* c, int32_t on) {
    if (!c) { thj_set_error("null ctx"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    if (!c->d_jb_key) { int rc = thj_juncbed_reset_async(c); if (rc) return rc; }
    if (c->jb_records) { thj_set_error("thj_juncbed_collect_indels: records were added already (call it between reset and the first add)"); return THJ_ESTATE; }
    if (on) { HIPCHK(hipStreamSynchronize(c->stream)); int rc = jbi_alloc(c); if (rc) return rc; }
    c->jbi_on = on != 0;
    return THJ_OK;
}

static JbfTable jbf_table(thj_ctx* c) {
    const int64_t n = c->jbf_cap;
    return JbfTable{c->d_jbf_u64, c->d_jbf_u64 + n, c->d_jbf_u32, c->d_jbf_u32 + n, c->d_jbf_u32 + 2 * n, (u64)n - 1, c->d_jbf_cnt};
}

extern "C" int thj_juncbed_collect_fusions(thj_ctx* c, int32_t on, int32_t anchor_len, int32_t read_mismatches, int32_t multireads) {
    if (!c) { thj_set_error("null ctx"); return THJ_EINVAL; }
    if (on && (anchor_len < 0 || read_mismatches < 0 || multireads < 0)) { thj_set_error("thj_juncbed_collect_fusions: bad argument (anchor_len, read_mismatches, multireads >= 0)"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    if (!c->d_jb_key) { int rc = thj_juncbed_reset_async(c); if (rc) return rc; }
    if (c->jb_records) { thj_set_error("thj_juncbed_collect_fusions: records were added already (call it between reset and the first add)"); return THJ_ESTATE; }
    c->jbf_on = false;
    if (!on) return THJ_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->jbf_cap != c->jb_cap || !c->d_jbf_u64) {                  // as many slots as the junction table has
        hipFree(c->d_jbf_u64); hipFree(c->d_jbf_u32);
        c->d_jbf_u64 = nullptr; c->d_jbf_u32 = nullptr; c->jbf_cap = 0;
        HIPCHK(hipMalloc(&c->d_jbf_u64, (size_t)c->jb_cap * 8 * 2));     // the two key words
        HIPCHK(hipMalloc(&c->d_jbf_u32, (size_t)c->jb_cap * 4 * 3));     // number in arrival order, pass-1 count, slots in arrival order
        c->jbf_cap = c->jb_cap;
    }
    if (!c->d_jbf_cnt) HIPCHK(hipMalloc(&c->d_jbf_cnt, JBF_N_COUNTERS * sizeof(unsigned long long)));
    HIPCHK(hipMemsetAsync(c->d_jbf_u64, 0xFF, (size_t)c->jbf_cap * 8 * 2, c->stream));
    HIPCHK(hipMemsetAsync(c->d_jbf_u32, 0, (size_t)c->jbf_cap * 4 * 3, c->stream));
    HIPCHK(hipMemsetAsync(c->d_jbf_cnt, 0, JBF_N_COUNTERS * sizeof(unsigned long long), c->stream));
    c->jbf_anchor = anchor_len; c->jbf_mismatches = read_mismatches; c->jbf_multireads = multireads;
    c->jbf_groups = 0; c->h_jbf.clear();
    c->jbf_on = true;
    return THJ_OK;
}

// the occurrence buffers are counted first, so that they are exactly large enough
template <class T>
static int jb_grow_occ(void*& buf, int64_t& cap, unsigned long long before, unsigned long long after) {
    if ((int64_t)after <= cap) return THJ_OK;
    const int64_t ncap = (int64_t)after + (int64_t)after / 4 + 4096;
    T* n = nullptr;
    HIPCHK(hipMalloc(&n, (size_t)ncap * sizeof(T)));
    if (buf && before) HIPCHK(hipMemcpy(n, buf, (size_t)before * sizeof(T), hipMemcpyDeviceToDevice));
    hipFree(buf);
    buf = n; cap = ncap;
    return THJ_OK;
}

// the fusion half of an add call, after the junction half: r's read_idx fields are below n_groups
static int jbf_add(thj_ctx* c, const JbRecs& r, int64_t n_groups) {
    const int64_t total = r.n_slots + r.n_extra;
    if (n_groups < 1) { thj_set_error("fusions are being collected: the add call knows no reads"); return THJ_EINVAL; }
    if (c->jbf_groups + n_groups > c->jbf_groups_cap) {             // [group sizes | records of the group the filter drops]
        const int64_t ncap = (c->jbf_groups + n_groups) + (c->jbf_groups + n_groups) / 4 + 4096;
        uint32_t* n = nullptr;
        HIPCHK(hipMalloc(&n, (size_t)ncap * 4 * 2));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (c->d_jbf_grp && c->jbf_groups) HIPCHK(hipMemcpy(n, c->d_jbf_grp, (size_t)c->jbf_groups * 4, hipMemcpyDeviceToDevice));
        hipFree(c->d_jbf_grp);
        c->d_jbf_grp = n; c->jbf_groups_cap = ncap;
    }
    uint32_t* grp1 = c->d_jbf_grp + c->jbf_groups;
    HIPCHK(hipMemsetAsync(grp1, 0, (size_t)n_groups * 4, c->stream));
    int64_t blocks = (total + 255) / 256; if (blocks > 4096) blocks = 4096;
    const Genome g{c->d_blocks, c->d_contig_blk, c->d_contig_len, c->n_contigs};
    const JbfCfg cfg{c->jbf_anchor, c->jbf_mismatches, c->jbf_multireads};
    unsigned long long before[JBF_N_COUNTERS] = {}, after[JBF_N_COUNTERS] = {};
    HIPCHK(hipMemcpyAsync(before, c->d_jbf_cnt, sizeof before, hipMemcpyDeviceToHost, c->stream));
    hipLaunchKernelGGL(thj_k_jbf_count, dim3((unsigned)blocks), dim3(256), 0, c->stream, g, r, cfg, grp1, (u64)n_groups, c->d_jbf_cnt);
    HIPCHK(hipMemcpyAsync(after, c->d_jbf_cnt, sizeof after, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    int rc = jb_grow_occ<JbfOcc>(c->d_jbf_focc, c->jbf_focc_cap, before[JBF_FOCC], after[JBF_FBOUND]);
    if (!rc) rc = jb_grow_occ<JbfUOcc>(c->d_jbf_uocc, c->jbf_uocc_cap, before[JBF_UOCC], after[JBF_UBOUND]);
    if (!rc) rc = jb_grow_occ<JbfJOcc>(c->d_jbf_jocc, c->jbf_jocc_cap, before[JBF_JOCC], after[JBF_JBOUND]);
    if (rc) return rc;
    const u64 grp_base = (u64)c->jbf_groups;
    c->jbf_groups += n_groups;
    hipLaunchKernelGGL(thj_k_jbf_add, dim3((unsigned)blocks), dim3(256), 0, c->stream, g, r, jb_table(c), jbf_table(c), cfg, (const uint32_t*)grp1, (u64)n_groups, grp_base,
                       (JbfOcc*)c->d_jbf_focc, (unsigned long long)c->jbf_focc_cap, (JbfUOcc*)c->d_jbf_uocc, (unsigned long long)c->jbf_uocc_cap,
                       (JbfJOcc*)c->d_jbf_jocc, (unsigned long long)c->jbf_jocc_cap);
    HIPCHK(hipGetLastError());
    return THJ_OK;
}

// n_groups: with fusions collected, the number of reads the records' read_idx fields count over
static int jb_add(thj_ctx* c, const JbRecs& r, const JbiSeq& sq = JbiSeq{}, int64_t n_groups = 0) {
    if (!c->d_jb_key) { int rc = thj_juncbed_reset_async(c); if (rc) return rc; }
    const int64_t total = r.n_slots + r.n_extra;
    if (total == 0) return THJ_OK;
    const bool indel = c->jbi_on;
    if (c->jb_records + total >= (1ll << 40)) { thj_set_error("more than 2^40 records in one consensus"); return THJ_EINVAL; }
    int64_t blocks = (total + 255) / 256; if (blocks > 4096) blocks = 4096;
    unsigned long long before[8] = {}, after[8] = {};
    HIPCHK(hipMemcpyAsync(before, c->d_jb_cnt, sizeof before, hipMemcpyDeviceToHost, c->stream));
    if (indel) hipLaunchKernelGGL(thj_k_jb_count<true>, dim3((unsigned)blocks), dim3(256), 0, c->stream, r, c->d_jb_cnt);
    else hipLaunchKernelGGL(thj_k_jb_count<false>, dim3((unsigned)blocks), dim3(256), 0, c->stream, r, c->d_jb_cnt);
    HIPCHK(hipMemcpyAsync(after, c->d_jb_cnt, sizeof after, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    int rc = jb_grow_occ<JbOcc>(c->d_jb_occ, c->jb_occ_cap, before[1], after[1]);
    if (!rc && indel) rc = jb_grow_occ<JbiOcc>(c->d_jbi_occ, c->jbi_occ_cap, before[4], after[4]);
    if (rc) return rc;
    const u64 ord_base = (u64)c->jb_records;
    c->jb_records += total;
    if (after[1] == before[1] && after[4] == before[4]) return c->jbf_on ? jbf_add(c, r, n_groups) : THJ_OK;
    Genome g{c->d_blocks, c->d_contig_blk, c->d_contig_len, c->n_contigs};
    if (indel) hipLaunchKernelGGL(thj_k_jb_add<true>, dim3((unsigned)blocks), dim3(256), 0, c->stream, g, r, jb_table(c), (JbOcc*)c->d_jb_occ, (unsigned long long)c->jb_occ_cap,
                                  sq, (JbiOcc*)c->d_jbi_occ, (unsigned long long)c->jbi_occ_cap, ord_base);
    else hipLaunchKernelGGL(thj_k_jb_add<false>, dim3((unsigned)blocks), dim3(256), 0, c->stream, g, r, jb_table(c), (JbOcc*)c->d_jb_occ, (unsigned long long)c->jb_occ_cap,
                            sq, (JbiOcc*)nullptr, 0ull, ord_base);
    HIPCHK(hipGetLastError());
    c->jb_occ_used = (int64_t)after[1];
    c->jbi_occ_used = (int64_t)after[4];
    return c->jbf_on ? jbf_add(c, r, n_groups) : THJ_OK;
}

extern "C" int thj_juncbed_add_span_async(thj_ctx* c) {
    if (!c) { thj_set_error("null ctx"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    if (c->jbi_on) { thj_set_error("thj_juncbed_add_span_async: indels are being collected, the records' bases are needed (thj_juncbed_add_span_seq_async)"); return THJ_EINVAL; }
    JbRecs r{(const OutAln*)c->d_aln_pool, c->d_nrec, c->span_reads, (const OutAln*)c->d_aln_sorted, c->n_ovf, true};
    return jb_add(c, r, JbiSeq{}, c->span_reads);
}

extern "C" int thj_juncbed_add_span_seq_async(thj_ctx* c, const thj_span_batch* batch) {
    if (!c || !batch) { thj_set_error("thj_juncbed_add_span_seq_async: bad argument"); return THJ_EINVAL; }
    if (!c->jbi_on) return thj_juncbed_add_span_async(c);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->n_alns == 0) return THJ_OK;
    if (!batch->read_planes || !batch->read_len || batch->words_per_plane < 1) { thj_set_error("thj_juncbed_add_span_seq_async: the batch holds no reads"); return THJ_EINVAL; }
    // the records in thj_span_download's order: that order says which of two insertions is the first
    void* d_alns = nullptr;
    int rc = thj_span_compact_device(c, &d_alns);
    if (rc == THJ_EFALLBACK) { thj_set_error("thj_juncbed_add_span_seq_async: the pass's records could not be put in order on the device"); return THJ_EFALLBACK; }
    if (rc) return rc;
    JbRecs r{(const OutAln*)d_alns, nullptr, c->n_alns, nullptr, 0, false};
    JbiSeq sq{nullptr, nullptr, (const u64*)batch->read_planes, batch->read_len, batch->words_per_plane, batch->n_reads};
    rc = jb_add(c, r, sq, c->span_reads);
    (void)hipStreamSynchronize(c->stream);
    thj_dev_release(c, d_alns);
    return rc;
}

// ref_id, n_cigar and -- for a fusion alignment -- ref_id2 of host records, before anything is launched
static int jb_check_records(thj_ctx* c, const thj_aln* recs, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (recs[i].ref_id < 1 || (int32_t)recs[i].ref_id > c->n_contigs || recs[i].n_cigar > 16) { thj_set_error("record %lld: contig or cigar out of range", (long long)i); return THJ_EINVAL; }
    if (c->jbf_on)
        for (int64_t i = 0; i < n; ++i) {
            if ((int64_t)recs[i].read_idx >= n) { thj_set_error("record %lld: read_idx %u, but the call has %lld records (fusions are being collected: read_idx numbers the reads of the call from 0)", (long long)i, recs[i].read_idx, (long long)n); return THJ_EINVAL; }
            jbw::FusionSite s;
            if (jbw::fusion(recs[i].cigar, recs[i].n_cigar, recs[i].left, recs[i].ref_id, s) && (s.ref1 < 1 || (int32_t)s.ref1 > c->n_contigs || s.ref2 < 1 || (int32_t)s.ref2 > c->n_contigs)) {
                thj_set_error("record %lld: the second contig of the fusion alignment is out of range", (long long)i); return THJ_EINVAL;
            }
        }
    return THJ_OK;
}
static int jb_add_host(thj_ctx* c, const thj_aln* recs, int64_t n, const int64_t* ins_off, const uint8_t* ins_bases) {
    void *tmp = nullptr, *d_off = nullptr, *d_bases = nullptr;
    auto done = [&](int code) { (void)hipStreamSynchronize(c->stream); hipFree(tmp); hipFree(d_off); hipFree(d_bases); return code; };
#define JB_HIP(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) { thj_set_error("%s: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); return done(THJ_EHIP); } } while (0)
    JB_HIP(hipMalloc(&tmp, (size_t)n * sizeof(thj_aln)));
    JB_HIP(hipMemcpyAsync(tmp, recs, (size_t)n * sizeof(thj_aln), hipMemcpyHostToDevice, c->stream));
    JbiSeq sq{};
    if (ins_off) {
        const size_t nb = (size_t)ins_off[n];
        JB_HIP(hipMalloc(&d_off, (size_t)(n + 1) * 8));
        JB_HIP(hipMalloc(&d_bases, nb + 16));
        JB_HIP(hipMemcpyAsync(d_off, ins_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, c->stream));
        if (nb) JB_HIP(hipMemcpyAsync(d_bases, ins_bases, nb, hipMemcpyHostToDevice, c->stream));
        sq.ins_off = (const int64_t*)d_off; sq.ins_bases = (const uint8_t*)d_bases;
    }
#undef JB_HIP
    JbRecs r{(const OutAln*)tmp, nullptr, n, nullptr, 0, false};
    return done(jb_add(c, r, sq, n));
}

extern "C" int thj_juncbed_add_records(thj_ctx* c, const thj_aln* recs, int64_t n, int32_t on_device) {
    if (!c || n < 0 || (n > 0 && !recs)) { thj_set_error("thj_juncbed_add_records: bad argument"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    if (n == 0) return THJ_OK;
    if (on_device) { JbRecs r{(const OutAln*)recs, nullptr, n, nullptr, 0, false}; return jb_add(c, r, JbiSeq{}, n); }
    if (const int rc = jb_check_records(c, recs, n)) return rc;
    if (c->jbi_on)
        for (int64_t i = 0; i < n; ++i)
            if (jbw::inss(recs[i].cigar, recs[i].n_cigar, recs[i].left, recs[i].ref_id, [](uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, int) {})) {
                thj_set_error("thj_juncbed_add_records: record %lld has an insertion and indels are being collected: its bases are needed (thj_juncbed_add_records_seq)", (long long)i);
                return THJ_EINVAL;
            }
    return jb_add_host(c, recs, n, nullptr, nullptr);
}

extern "C" int thj_juncbed_add_records_seq(thj_ctx* c, const thj_aln* recs, int64_t n, const int64_t* ins_off, const char* ins_bases) {
    if (!c || n < 0 || (n > 0 && (!recs || !ins_off))) { thj_set_error("thj_juncbed_add_records_seq: bad argument"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    if (n == 0) return THJ_OK;
    if (const int rc = jb_check_records(c, recs, n)) return rc;
    if (ins_off[0] != 0 || (ins_off[n] > 0 && !ins_bases)) { thj_set_error("thj_juncbed_add_records_seq: bad argument (ins_off[0] must be 0)"); return THJ_EINVAL; }
    // everything is looked at before anything is counted
    for (int64_t i = 0; i < n; ++i) {
        int64_t at = ins_off[i]; bool bad_ref = false; uint32_t too_long = 0;
        if (ins_off[i + 1] < at) { thj_set_error("thj_juncbed_add_records_seq: ins_off falls at record %lld", (long long)i); return THJ_EINVAL; }
        jbw::inss(recs[i].cigar, recs[i].n_cigar, recs[i].left, recs[i].ref_id, [&](uint32_t ref, uint32_t, uint32_t len, uint32_t, uint32_t, uint32_t, int) {
            if (ref < 1 || (int32_t)ref > c->n_contigs) bad_ref = true;
            if (len > (uint32_t)JBI_MAX_INS) too_long = len;
            at += len;
        });
        jbw::dels(recs[i].cigar, recs[i].n_cigar, recs[i].left, recs[i].ref_id, [&](uint32_t ref, uint32_t, uint32_t, uint32_t, uint32_t, int) { if (ref < 1 || (int32_t)ref > c->n_contigs) bad_ref = true; });
        if (bad_ref) { thj_set_error("record %lld: the second contig of the fusion alignment is out of range", (long long)i); return THJ_EINVAL; }
        if (too_long) { thj_set_error("record %lld: an insertion of %u bases (at most %d are held)", (long long)i, too_long, JBI_MAX_INS); return THJ_EINVAL; }
        if (at != ins_off[i + 1]) { thj_set_error("record %lld: %lld inserted bases in its cigar, %lld handed in", (long long)i, (long long)(at - ins_off[i]), (long long)(ins_off[i + 1] - ins_off[i])); return THJ_EINVAL; }
        for (int64_t k = ins_off[i]; k < at; ++k)
            if (!strchr("ACGTN", ins_bases[k]) || !ins_bases[k]) { thj_set_error("record %lld: inserted base '%c' (A, C, G, T and N are held)", (long long)i, ins_bases[k]); return THJ_EINVAL; }
    }
    return jb_add_host(c, recs, n, ins_off, (const uint8_t*)ins_bases);
}

// contig (1-based) and contig-relative coordinate of a key's global coordinate + 1: a contig's blocks are followed by a guard
// block, so start .. start + length (left = -1 .. length - 1) belongs to it alone
static void jb_locate(thj_ctx* c, u64 gp1, uint32_t* ref_id, uint32_t* left) {
    int lo = 0, hi = c->n_contigs;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if ((u64)c->h_contig_blk[(size_t)mid] * 64 <= gp1) lo = mid; else hi = mid; }
    *ref_id = (uint32_t)lo + 1; *left = (uint32_t)(gp1 - (u64)c->h_contig_blk[(size_t)lo] * 64 - 1);
}

// the indel half of finish: tables from scratch, second pass, letters, both sets in their own order
static int jbi_finish(thj_ctx* c) {
    c->h_jbi_ins.clear(); c->h_jbi_del.clear();
    if (!c->jbi_on) return THJ_OK;
    HIPCHK(hipMemsetAsync(c->d_jbi_u64, 0xFF, (size_t)c->jbi_cap * 8 * 8, c->stream));
    HIPCHK(hipMemsetAsync(c->d_jbi_u32, 0, (size_t)c->jbi_cap * 4 * 6, c->stream));
    HIPCHK(hipMemsetAsync(c->d_jbi_cnt, 0, 4 * sizeof(unsigned long long), c->stream));
    JbiTable td = jbi_table(c, 0), ti = jbi_table(c, 1);
    if (c->jbi_occ_used) {
        int64_t b = (c->jbi_occ_used + 255) / 256; if (b > 4096) b = 4096;
        hipLaunchKernelGGL(thj_k_jbi_second, dim3((unsigned)b), dim3(256), 0, c->stream, td, ti, (const JbiOcc*)c->d_jbi_occ, c->jbi_occ_used, (const JbOcc*)c->d_jb_occ, c->jb_occ_used,
                           (const uint32_t*)(c->d_jb_u32 + 8 * c->jb_cap));
        hipLaunchKernelGGL(thj_k_jbi_letters, dim3((unsigned)b), dim3(256), 0, c->stream, ti, (const JbiOcc*)c->d_jbi_occ, c->jbi_occ_used);
        HIPCHK(hipGetLastError());
    }
    unsigned long long h[4];
    HIPCHK(hipMemcpyAsync(h, c->d_jbi_cnt, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int64_t room = c->jbi_cap - c->jbi_cap / 4;
    if (h[2] || (int64_t)h[0] > room || (int64_t)h[1] > room) {
        thj_set_error("indel table full (%llu distinct deletions, %llu distinct insertions, capacity %lld each): call thj_juncbed_configure with a larger capacity and add the records again",
                      h[0], h[1], (long long)c->jbi_cap);
        return THJ_EOVERFLOW;
    }
    for (int which = 0; which < 2; ++which) {
        const int64_t n = (int64_t)h[which];
        if (!n) continue;
        const JbiTable t = which ? ti : td;
        size_t need = 0;
        HIPCHK(hipcub::DeviceRadixSort::SortKeys(nullptr, need, (const u64*)t.list, c->d_jb_sorted, n, 0, 64, c->stream));
        if (const int e = ensure_sort_tmp(c, need)) return e;
        size_t bytes = c->sort_tmp_bytes;
        HIPCHK(hipcub::DeviceRadixSort::SortKeys(c->d_sort_tmp, bytes, (const u64*)t.list, c->d_jb_sorted, n, 0, 64, c->stream));
        JbiOut* d_out = nullptr;
        HIPCHK(hipMalloc(&d_out, (size_t)n * sizeof(JbiOut)));
        int64_t b = (n + 255) / 256; if (b > 4096) b = 4096;
        hipLaunchKernelGGL(thj_k_jbi_gather, dim3((unsigned)b), dim3(256), 0, c->stream, t, (const u64*)c->d_jb_sorted, n, d_out);
        std::vector<JbiOut> out((size_t)n);
        const hipError_t e1 = hipMemcpyAsync(out.data(), d_out, (size_t)n * sizeof(JbiOut), hipMemcpyDeviceToHost, c->stream);
        const hipError_t e2 = hipStreamSynchronize(c->stream);
        hipFree(d_out);
        HIPCHK(e1); HIPCHK(e2);
        for (auto& o : out) {
            uint32_t ref_id, left;
            jb_locate(c, o.key >> 30, &ref_id, &left);
            if (which) {
                thj_insstat s; memset(&s, 0, sizeof s);
                s.ref_id = ref_id; s.left = left; s.len = (uint32_t)(o.key & 0xFFu); s.support = o.support; s.left_extent = o.le; s.right_extent = o.re;
                for (uint32_t k = 0; k < s.len && k < (uint32_t)JBI_MAX_INS; ++k) s.bases[k] = "ACGTN???"[(o.bases >> (3 * k)) & 7u];
                c->h_jbi_ins.push_back(s);
            } else {
                thj_juncstat s;
                s.ref_id = ref_id; s.left = left; s.right = left + (uint32_t)((o.key >> 1) & ((1ull << 29) - 1)); s.antisense = 0;
                s.left_extent = o.le; s.right_extent = o.re; s.support = o.support; s.reserved = 0;
                c->h_jbi_del.push_back(s);
            }
        }
    }
    return THJ_OK;
}

// the fusion half of finish, after acc2 is known: drops, pass 2, the pass-1 set's ends, unsupport, rows
static int jbf_finish(thj_ctx* c) {
    c->h_jbf.clear();
    if (!c->jbf_on) return THJ_OK;
    unsigned long long h[JBF_N_COUNTERS];
    HIPCHK(hipMemcpyAsync(h, c->d_jbf_cnt, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (h[JBF_FLAGS]) { thj_set_error("thj_juncbed_finish: the fusions of the records added cannot be counted: a record points outside the reads of its add call or outside the genome"); return THJ_EINVAL; }
    if (h[JBF_OVERFLOW] || (int64_t)h[JBF_DISTINCT] > c->jbf_cap - c->jbf_cap / 4) {
        thj_set_error("fusion table full (%llu distinct fusions, capacity %lld): call thj_juncbed_configure with a larger capacity and add the records again", h[JBF_DISTINCT], (long long)c->jbf_cap);
        return THJ_EOVERFLOW;
    }
    const int64_t n_f = (int64_t)h[JBF_DISTINCT], n_focc = (int64_t)h[JBF_FOCC], n_uocc = (int64_t)h[JBF_UOCC], n_jocc = (int64_t)h[JBF_JOCC];
    if (!n_f) return THJ_OK;
    const JbfTable t = jbf_table(c);
    uint32_t *grp1 = c->d_jbf_grp, *gdrop = c->d_jbf_grp + c->jbf_groups_cap;
    // one block of scratch: statistics, rows, the ends and their sorted copy
    const size_t b_st = ((size_t)n_f * sizeof(JbfStat) + 15) & ~(size_t)15, b_out = ((size_t)n_f * sizeof(thj_fusstat) + 15) & ~(size_t)15, b_key = (size_t)n_f * 2 * 8, b_val = (size_t)n_f * 2 * 4;
    char* d = nullptr;
    HIPCHK(hipMalloc(&d, b_st + b_out + 2 * b_key + 2 * b_val));
    JbfStat* st = (JbfStat*)d; thj_fusstat* out = (thj_fusstat*)(d + b_st);
    u64 *k_in = (u64*)(d + b_st + b_out), *k_out = k_in + n_f * 2; uint32_t *v_in = (uint32_t*)(k_out + n_f * 2), *v_out = v_in + n_f * 2;
    std::vector<thj_fusstat> rows((size_t)n_f);
    int64_t n_ends = 0;
    auto run = [&]() -> int {
        HIPCHK(hipMemsetAsync(st, 0, b_st, c->stream));
        HIPCHK(hipMemsetAsync(gdrop, 0, (size_t)c->jbf_groups * 4, c->stream));
        HIPCHK(hipMemsetAsync(&c->d_jbf_cnt[JBF_ENDS], 0, sizeof(unsigned long long), c->stream));
        auto grid = [](int64_t n) { int64_t b = (n + 255) / 256; return dim3((unsigned)(b > 4096 ? 4096 : b)); };
        if (n_jocc) hipLaunchKernelGGL(thj_k_jbf_drop, grid(n_jocc), dim3(256), 0, c->stream, (JbfJOcc*)c->d_jbf_jocc, n_jocc, (const uint32_t*)(c->d_jb_u32 + 8 * c->jb_cap), gdrop);
        if (n_focc) hipLaunchKernelGGL(thj_k_jbf_second, grid(n_focc), dim3(256), 0, c->stream, t, (const JbfOcc*)c->d_jbf_focc, n_focc, (const JbfJOcc*)c->d_jbf_jocc, n_jocc,
                                       (const uint32_t*)grp1, (const uint32_t*)gdrop, (int)c->jbf_multireads, st);
        hipLaunchKernelGGL(thj_k_jbf_ends, grid(n_f), dim3(256), 0, c->stream, t, n_f, k_in, v_in);
        unsigned long long ne = 0;
        HIPCHK(hipMemcpyAsync(&ne, &c->d_jbf_cnt[JBF_ENDS], sizeof ne, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        n_ends = (int64_t)ne;
        if (n_ends && n_uocc) {
            size_t need = 0;
            HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, need, (const u64*)k_in, k_out, (const uint32_t*)v_in, v_out, n_ends, 0, 64, c->stream));
            if (const int e = ensure_sort_tmp(c, need)) return e;
            size_t bytes = c->sort_tmp_bytes;
            HIPCHK(hipcub::DeviceRadixSort::SortPairs(c->d_sort_tmp, bytes, (const u64*)k_in, k_out, (const uint32_t*)v_in, v_out, n_ends, 0, 64, c->stream));
            hipLaunchKernelGGL(thj_k_jbf_unsupport, grid(n_uocc), dim3(256), 0, c->stream, (const JbfUOcc*)c->d_jbf_uocc, n_uocc, (const uint32_t*)grp1, (const uint32_t*)gdrop,
                               (int)c->jbf_multireads, (const u64*)k_out, (const uint32_t*)v_out, n_ends, st);
        }
        const Genome g{c->d_blocks, c->d_contig_blk, c->d_contig_len, c->n_contigs};
        hipLaunchKernelGGL(thj_k_jbf_gather, dim3((unsigned)(n_f > 4096 ? 4096 : n_f)), dim3(256), 0, c->stream, g, t, (const JbfStat*)st, n_f, out);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(rows.data(), out, (size_t)n_f * sizeof(thj_fusstat), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return THJ_OK;
    };
    const int rc = run();
    hipFree(d);
    if (rc) return rc;
    for (auto& r : rows) {
        if (!r.count) continue;                                                           // print_fusions: count > 0 only
        if (!n_ends) {
            // an empty pass-1 set: the reference's second pass then runs like its first (update_stat = fusions_ref.size() > 0,
            // tophat_reports.cpp:1167) and only counts
            r.unsupport = r.left_ext = r.right_ext = r.n_diffs = 0;
            memset(r.diffs, 0, sizeof r.diffs); memset(r.left_bases, 0, sizeof r.left_bases); memset(r.right_bases, 0, sizeof r.right_bases);
            memset(r.seq1, 0, sizeof r.seq1); memset(r.seq2, 0, sizeof r.seq2);
        }
        c->h_jbf.push_back(r);
    }
    std::sort(c->h_jbf.begin(), c->h_jbf.end(), [](const thj_fusstat& a, const thj_fusstat& b) {      // Fusion::operator<, fusions.h:39-67
        return std::make_tuple(a.ref_id1, a.ref_id2, a.left, a.right, a.dir) < std::make_tuple(b.ref_id1, b.ref_id2, b.left, b.right, b.dir);
    });
    return THJ_OK;
}

// the junction half of finish, n > 0 distinct junctions: filters (acc2), second pass, final set
static int jb_finish_juncs(thj_ctx* c, int64_t n, int32_t min_anchor_len) {
    JbTable t = jb_table(c);
    uint32_t* acc2 = c->d_jb_u32 + 8 * c->jb_cap;
    int64_t blocks = (c->jb_cap + 255) / 256; if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(thj_k_jb_accept, dim3((unsigned)blocks), dim3(256), 0, c->stream, t, n, (int)min_anchor_len);
    size_t need = 0;
    HIPCHK(hipcub::DeviceRadixSort::SortKeys(nullptr, need, (const u64*)c->d_jb_list, c->d_jb_sorted, n, 0, 64, c->stream));
    if (const int e = ensure_sort_tmp(c, need)) return e;
    size_t bytes = c->sort_tmp_bytes;
    HIPCHK(hipcub::DeviceRadixSort::SortKeys(c->d_sort_tmp, bytes, (const u64*)c->d_jb_list, c->d_jb_sorted, n, 0, 64, c->stream));
    int64_t b2 = (n + 255) / 256; if (b2 > 4096) b2 = 4096;
    hipLaunchKernelGGL(thj_k_jb_knockout, dim3((unsigned)b2), dim3(256), 0, c->stream, t, (const u64*)c->d_jb_sorted, n, (int)min_anchor_len, acc2);
    // second pass (cnt2 / le2 / re2 start from zero: a finish can be repeated)
    HIPCHK(hipMemsetAsync(t.cnt2, 0, (size_t)c->jb_cap * 4 * 3, c->stream));
    if (c->jb_occ_used) {
        int64_t b3 = (c->jb_occ_used + 255) / 256; if (b3 > 4096) b3 = 4096;
        hipLaunchKernelGGL(thj_k_jb_second, dim3((unsigned)b3), dim3(256), 0, c->stream, t, (const JbOcc*)c->d_jb_occ, c->jb_occ_used, (const uint32_t*)acc2);
    }
    JbOut* d_out = nullptr;
    HIPCHK(hipMalloc(&d_out, (size_t)n * sizeof(JbOut)));
    hipLaunchKernelGGL(thj_k_jb_gather, dim3((unsigned)b2), dim3(256), 0, c->stream, t, (const u64*)c->d_jb_sorted, n, d_out);
    HIPCHK(hipGetLastError());
    std::vector<JbOut> out((size_t)n);
    HIPCHK(hipMemcpyAsync(out.data(), d_out, (size_t)n * sizeof(JbOut), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    hipFree(d_out);
    for (auto& o : out) {
        if (o.support == 0 || o.le < 8 || o.re < 8) continue;                          // tophat_reports.cpp:2974-2984
        thj_juncstat s;
        const int64_t gp = (int64_t)(o.key >> 30) - 1;                                   // global coordinate of `left`
        int lo = 0, hi = c->n_contigs;
        const int64_t start = gp - (int64_t)o.left;                                      // = contig start (left is contig-relative)
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if ((int64_t)c->h_contig_blk[(size_t)mid] * 64 <= start) lo = mid; else hi = mid; }
        s.ref_id = (uint32_t)lo + 1; s.left = o.left; s.right = o.left + (uint32_t)((o.key >> 1) & ((1ull << 29) - 1)); s.antisense = (uint32_t)(o.key & 1ull);
        s.left_extent = o.le; s.right_extent = o.re; s.support = o.support; s.reserved = 0;
        c->h_jb.push_back(s);
    }
    return THJ_OK;
}

extern "C" int thj_juncbed_finish(thj_ctx* c, int32_t min_anchor_len, int64_t* n_juncs) {
    if (!c || min_anchor_len < 0 || min_anchor_len > 60) { thj_set_error("thj_juncbed_finish: bad argument (min_anchor_len 0..60)"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    c->h_jb.clear(); c->h_jbi_ins.clear(); c->h_jbi_del.clear(); c->h_jbf.clear();
    if (n_juncs) *n_juncs = 0;
    if (!c->d_jb_key) return THJ_OK;
    unsigned long long h[8];
    HIPCHK(hipMemcpyAsync(h, c->d_jb_cnt, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (h[3] || (int64_t)h[0] > c->jb_cap - c->jb_cap / 4) {
        thj_set_error("junction table full (%llu distinct junctions, capacity %lld): call thj_juncbed_configure with a larger capacity and add the records again",
                      h[0], (long long)c->jb_cap);
        return THJ_EOVERFLOW;
    }
    if (c->jbi_on && h[6]) {
        thj_set_error("thj_juncbed_finish: the indels of the records added cannot be counted:%s%s%s",
                      h[6] & JBI_FLAG_LONG ? " an insertion is longer than the 16 bases that are held;" : "",
                      h[6] & JBI_FLAG_RANGE ? " a record points outside the genome, its batch or its bases;" : "",
                      h[6] & JBI_FLAG_NOSEQ ? " a record with an insertion came without bases;" : "");
        return THJ_EINVAL;
    }
    const int64_t n = (int64_t)h[0];
    if (n) { const int rc = jb_finish_juncs(c, n, min_anchor_len); if (rc) return rc; }
    if (const int rc = jbi_finish(c)) { c->h_jb.clear(); return rc; }
    if (const int rc = jbf_finish(c)) { c->h_jb.clear(); c->h_jbi_ins.clear(); c->h_jbi_del.clear(); return rc; }
    if (n_juncs) *n_juncs = (int64_t)c->h_jb.size();
    return THJ_OK;
}

extern "C" int thj_juncbed_download(thj_ctx* c, thj_juncstat* out) {
    if (!c || (!c->h_jb.empty() && !out)) { thj_set_error("thj_juncbed_download: bad argument"); return THJ_EINVAL; }
    if (!c->h_jb.empty()) memcpy(out, c->h_jb.data(), c->h_jb.size() * sizeof(thj_juncstat));
    return THJ_OK;
}

extern "C" int thj_juncbed_indel_counts(thj_ctx* c, int64_t* n_ins, int64_t* n_del) {
    if (!c) { thj_set_error("null ctx"); return THJ_EINVAL; }
    if (n_ins) *n_ins = (int64_t)c->h_jbi_ins.size();
    if (n_del) *n_del = (int64_t)c->h_jbi_del.size();
    return THJ_OK;
}

extern "C" int thj_juncbed_indel_download(thj_ctx* c, thj_insstat* ins, thj_juncstat* dels) {
    if (!c || (!c->h_jbi_ins.empty() && !ins) || (!c->h_jbi_del.empty() && !dels)) { thj_set_error("thj_juncbed_indel_download: bad argument"); return THJ_EINVAL; }
    if (!c->h_jbi_ins.empty()) memcpy(ins, c->h_jbi_ins.data(), c->h_jbi_ins.size() * sizeof(thj_insstat));
    if (!c->h_jbi_del.empty()) memcpy(dels, c->h_jbi_del.data(), c->h_jbi_del.size() * sizeof(thj_juncstat));
    return THJ_OK;
}

extern "C" int thj_juncbed_fusion_count(thj_ctx* c, int64_t* n) {
    if (!c) { thj_set_error("null ctx"); return THJ_EINVAL; }
    if (n) *n = (int64_t)c->h_jbf.size();
    return THJ_OK;
}

extern "C" int thj_juncbed_fusion_download(thj_ctx* c, thj_fusstat* out) {
    if (!c || (!c->h_jbf.empty() && !out)) { thj_set_error("thj_juncbed_fusion_download: bad argument"); return THJ_EINVAL; }
    if (!c->h_jbf.empty()) memcpy(out, c->h_jbf.data(), c->h_jbf.size() * sizeof(thj_fusstat));
    return THJ_OK;
}
