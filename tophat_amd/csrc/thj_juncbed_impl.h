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
// Two switches, both set between reset and the first add (the decisions themselves: thj_jbknown_core.h).  The annotated junctions
// (thj_juncbed_known_junctions, tophat_reports --gtf-juncs): a sorted array of keys that the accept kernel looks every distinct junction
// up in; a junction found there is accepted as it is and marked (acc = jbk::ACC_KNOWN), and the knockout kernel leaves a marked
// junction alone.  The read filter (thj_juncbed_read_filter): jb_rec, through which every count and add kernel fetches its records,
// hands out nothing for a record over the limits, so such a record is gone for every set and both passes.
// A third (thj_juncbed_best_alignments): only each read's best alignments count -- thj_juncbed_best_impl.h; for paired input
// (thj_juncbed_pair_alignments, thj_juncbed_add_pairs) the inserts are graded first -- thj_juncbed_pair_impl.h.  And with that choice made
// (thj_juncbed_collect_accepted): finish leaves the scores, the reporting reads before every record and the generator's draws on the
// device, for the pass that writes the reported alignments out as BAM records afterwards (thj_juncbed_report_bam, thj_accepted.hip).
//
// Included at the end of thj_span.hip.  Not part of the timed hot path of bench.py unless asked for.
#pragma once
#include <tuple>
#include "thj_jb_walk.h"
#include "thj_jbknown_core.h"

// ord_hi / ord_lo: with best alignments chosen, the ordinal of the occurrence's record (its keep flag); 0 otherwise
struct JbOcc { uint32_t slot; uint16_t le, re; uint8_t nj, idx; uint16_t ord_hi; uint32_t ord_lo; };      // 16 bytes
static_assert(sizeof(JbOcc) == 16, "occurrence layout");

// A table's storage is declared once: its u64 columns (0xFF after a reset: the empty key), its uint32 columns (0 after a reset), its
// counters, and how many such tables lie side by side in one JbStore.  jb_store_alloc, jb_store_reset and the carving (jb_table,
// jbi_table, jbf_table, through jb_col64 / jb_col32) read these declarations; nobody else knows a column count.
struct JbLayout { int n64, n32, n_cnt, tables; };

enum { JB_KEY, JB_LIST, JB_N64 };                                                    // list: distinct keys in arrival order
// cnt2 le2 re2: the second pass; acc: what filter_junctions' loop decided, a value of jbk::ACC_* (ACC_KNOWN: accepted and marked gtf_match); acc2: 0 / 1 after the knockout
enum { JB_CNT1, JB_LE1, JB_RE1, JB_CNT2, JB_LE2, JB_RE2, JB_LEFT, JB_ACC, JB_ACC2, JB_N32 };
// counters: distinct keys, occurrences counted / written, overflow flag, indel occurrences counted / written, JBI_FLAG_* (thj_juncbed_indel_impl.h)
enum { JB_DISTINCT, JB_OCC_COUNTED, JB_OCC_WRITTEN, JB_OVERFLOW, JB_IOCC_COUNTED, JB_IOCC_WRITTEN, JB_IFLAGS, JB_N_COUNTERS = 8 };
static constexpr JbLayout JB_LAYOUT{JB_N64, JB_N32, JB_N_COUNTERS, 1};

struct JbTable {
    u64* key; u64 mask;
    uint32_t *cnt1, *le1, *re1, *cnt2, *le2, *re2, *left, *acc, *acc2;
    u64* list;
    unsigned long long* counters;
};

__device__ __forceinline__ u64 jb_mix(u64 x) { x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull; x ^= x >> 27; x *= 0x94d049bb133111ebull; x ^= x >> 31; return x; }

// The one-word tables (junctions, deletions, insertions): linear probing over all mask + 1 slots.  Whoever puts a key into an empty
// slot lists it and is told so (created), so that a caller can fill the slot's other columns.
struct JbSlot { uint32_t slot; bool created; };
__device__ __forceinline__ JbSlot jb_insert(u64* key, u64 mask, u64* list, unsigned long long* distinct, unsigned long long* overflow, u64 k) {
    u64 h = jb_mix(k) & mask;
    for (u64 probe = 0; probe <= mask; ++probe) {
        u64 cur = __hip_atomic_load(&key[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bool created = false;
        if (cur == ~0ull) {
            const u64 old = atomicCAS((unsigned long long*)&key[h], ~0ull, k);
            if (old == ~0ull) { const unsigned long long pos = atomicAdd(distinct, 1ull); if (pos <= mask) list[pos] = k; created = true; cur = k; }
            else cur = old;
        }
        if (cur == k) return JbSlot{(uint32_t)h, created};
        h = (h + 1) & mask;
    }
    atomicExch(overflow, 1ull);
    return JbSlot{0xFFFFFFFFu, false};
}
__device__ __forceinline__ uint32_t jb_find(const u64* key, u64 mask, u64 k) {
    u64 h = jb_mix(k) & mask;
    for (u64 probe = 0; probe <= mask; ++probe) {
        const u64 cur = key[h];
        if (cur == k) return (uint32_t)h;
        if (cur == ~0ull) return 0xFFFFFFFFu;
        h = (h + 1) & mask;
    }
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

// record i of a pass: slots (first record of every read that has one) then the extra pool; or a plain array.  flt: the read filter
// (jb_add fills it in); a record it drops is no record
// unflt (inserts are graded; null otherwise): record i is taken although the filter drops it -- the first pass of an insert without a pair
struct JbRecs { const OutAln* slots; const uint8_t* nrec; int64_t n_slots; const OutAln* extra; int64_t n_extra; bool slot_layout; jbk::ReadFilter flt; const uint8_t* unflt = nullptr; };
__device__ __forceinline__ const OutAln* jb_rec(const JbRecs& r, int64_t i) {
    const OutAln* a = i >= r.n_slots ? &r.extra[i - r.n_slots] : (!r.nrec || r.nrec[i]) ? &r.slots[i] : nullptr;
    if (r.flt.on && a && !(r.unflt && r.unflt[i]) && jbk::dropped(r.flt, a->mismatches, a->n_cigar < SPAN_MAXC ? a->n_cigar : SPAN_MAXC, JbCigar{(const uint32_t*)a, r.slot_layout})) a = nullptr;
    return a;
}

#include "thj_juncbed_indel_impl.h"

// INDEL: the records' DEL / dEL / INS / iNS ops are counted too (JB_IOCC_COUNTED; plain arrays only)
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
    if (threadIdx.x == 0 && s_n) atomicAdd(&counters[JB_OCC_COUNTED], (unsigned long long)s_n);
    if (INDEL && threadIdx.x == 0 && s_i) atomicAdd(&counters[JB_IOCC_COUNTED], (unsigned long long)s_i);
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

#include "thj_juncbed_best_impl.h"

// INDEL: beside the junction occurrences the records' indel occurrences are listed (iocc; record i of this call has ordinal ord_base + i)
// brec (best alignments are chosen; null otherwise): what thj_k_jbb_rank kept of this call's records.  A pass-1 duplicate adds nothing to
// the first-pass statistics (its junctions still get their slots); every record learns where its occurrences start, every occurrence
// its record and -- skey -- the key the score will look up.  mult (inserts are graded; null otherwise): how many times record i counts in the
// first pass -- the kept pairs it is in; JBP_SINGLE_END: the single-end rule.
template <bool INDEL>
__global__ __launch_bounds__(256) void thj_k_jb_add(Genome g, JbRecs r, JbTable t, JbOcc* occ, unsigned long long occ_cap,
                                                    JbiSeq sq, JbiOcc* iocc, unsigned long long iocc_cap, u64 ord_base, JbbRec* brec, u64* skey, const uint32_t* mult) {
    const int lane = threadIdx.x & 63;
    const int64_t total = r.n_slots + r.n_extra;
    // whole waves walk together so that the wave-wide reservations below see every lane
    const int64_t n_iter = (total + (int64_t)gridDim.x * blockDim.x - 1) / ((int64_t)gridDim.x * blockDim.x);
    for (int64_t it = 0; it < n_iter; ++it) {
        const int64_t i = it * (int64_t)gridDim.x * blockDim.x + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        const OutAln* a = i < total ? jb_rec(r, i) : nullptr;
        unsigned int nj = a ? (unsigned)jb_rec_juncs(*a, r.slot_layout, [](uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) {}) : 0u;
        const unsigned long long first = jb_wave_reserve(&t.counters[JB_OCC_WRITTEN], nj, lane);
        if (nj) {
            unsigned long long at = first;
            const bool anti = (a->flags & 4u) != 0;             // THJ_HIT_ANTISENSE_SPLICE
            uint8_t idx = 0;
            const uint8_t n8 = (uint8_t)nj;
            uint32_t counts = !brec || !(brec[i].flags & JBB_DUP1) ? 1u : 0u;
            if (mult && mult[i] != 0xFFFFFFFFu) counts = mult[i];
            const u64 ord = brec ? ord_base + (u64)i : 0ull;
            if (brec) { brec[i].jfirst = first; brec[i].nj = n8; }
            jb_rec_juncs(*a, r.slot_layout, [&](uint32_t ref, uint32_t left, uint32_t right, uint32_t le, uint32_t re) {
                const JbSlot ins = jb_insert(t.key, t.mask, t.list, &t.counters[JB_DISTINCT], &t.counters[JB_OVERFLOW], junc_key(g, ref, left, right, anti));
                const uint32_t slot = ins.slot;
                if (ins.created) t.left[slot] = left;
                if (slot != 0xFFFFFFFFu && counts) {
                    atomicAdd(&t.cnt1[slot], counts);
                    atomicMax(&t.le1[slot], le);
                    atomicMax(&t.re1[slot], re);
                }
                if (at < occ_cap) occ[at] = JbOcc{slot, (uint16_t)(le > 65535u ? 65535u : le), (uint16_t)(re > 65535u ? 65535u : re), n8, idx, (uint16_t)(ord >> 32), (uint32_t)ord};
                ++at; ++idx;
            });
            if (brec) {
                unsigned long long k = first;
                jbb::score_juncs(a->n_cigar < SPAN_MAXC ? a->n_cigar : SPAN_MAXC, a->left, JbCigar{(const uint32_t*)a, r.slot_layout},
                                 [&](uint32_t left, uint32_t right) { if (k < occ_cap) skey[k] = jbb_score_key(g, a->ref_id, left, right, anti); ++k; });
            }
        }
        if (INDEL) {
            const unsigned int ni = a ? (unsigned)jbi_rec_count(*a) : 0u;
            const unsigned long long iat = jb_wave_reserve(&t.counters[JB_IOCC_WRITTEN], ni, lane);
            if (ni) jbi_rec_write(g, *a, i, ord_base + (u64)i, nj ? (u64)first : JBI_NO_JUNC, sq, iocc, iat, iocc_cap, &t.counters[JB_IFLAGS]);
        }
    }
}

// the loop of filter_junctions (junctions.cpp:305-315) per distinct junction: accept_if_valid (:192-242), or -- a junction of the
// annotation, known[0 .. n_known) sorted -- accepted as it is and marked.  acc takes a value of jbk::ACC_*.
// Only junctions that a record shows have a slot.  The reference also holds the annotated junctions nobody shows: merge_with(junctions,
// gtf_junctions) puts them into the first-pass set with support 0 (tophat_reports.cpp:2814).  There they can knock nothing out
// (knockout_shadow_junctions asks junc_support < itr2->supporting_hits, and no support is below 0), no record is kept or dropped on
// their account (a record is asked about its own junctions only), and the final filter erases them (supporting_hits == 0, :2977).
// So no slot is made for them, and the table holds what it held without the annotation.
__global__ __launch_bounds__(256) void thj_k_jb_accept(JbTable t, int64_t n, int min_anchor, const u64* known, int64_t n_known) {
    if (n_known <= 0) known = nullptr;                         // no annotation: nothing is looked up
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= (int64_t)t.mask; i += (int64_t)gridDim.x * blockDim.x) {
        const u64 k = t.key[i];
        if (k == ~0ull) continue;
        uint32_t acc = jbk::accept(k, t.le1[i], t.re1[i], t.cnt1[i], min_anchor, known, n_known);
        // only pass-1 duplicates show it (best alignments): it is not in the first-pass set unless the annotation holds it
        if (t.cnt1[i] == 0u && acc != jbk::ACC_KNOWN) acc = jbk::ACC_REJECTED;
        t.acc[i] = acc;
    }
    (void)n;
}

// knockout_shadow_junctions (junctions.cpp:244-315) over the sorted distinct keys: an accepted junction loses to a junction of
// the other strand that starts within min_anchor_len before it (or at it, ending within min_anchor_len after it) when that
// one has more support.  Writes acc2 (the junction's own flag only, as the reference does).  any_known: some junction may be marked
// as annotated; such a one is not looked at (:270: accepted && !gtf_match) -- as somebody else's neighbour it competes with its support
// like any other.
__global__ __launch_bounds__(256) void thj_k_jb_knockout(JbTable t, const u64* sorted, int64_t n, int min_anchor, uint32_t* acc2, bool any_known) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const u64 k = sorted[i];
        const uint32_t si = jb_find(t.key, t.mask, k);
        const uint32_t acc = t.acc[si];
        uint32_t ok = jbk::accepted(acc) ? 1u : 0u;
        if (ok && !(any_known && jbk::exempt(acc)) && t.left[si] >= (uint32_t)min_anchor) {        // left < anchor: the reference's unsigned left wraps, the range is empty
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
                    const uint32_t s2 = jb_find(t.key, t.mask, k2);
                    if (my_support < t.cnt1[s2]) ok = 0;
                }
            }
        }
        acc2[si] = ok;
    }
}

// second pass: the first occurrence of a record speaks for the record.  keep (best alignments; null otherwise): the records' keep flags;
// pcnt (inserts are graded; null otherwise): the reported pairs a record is in -- it counts once per pair
__global__ __launch_bounds__(256) void thj_k_jb_second(JbTable t, const JbOcc* occ, int64_t n_occ, const uint32_t* acc2, const uint8_t* keep, const uint32_t* pcnt) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_occ; i += (int64_t)gridDim.x * blockDim.x) {
        const JbOcc o = occ[i];
        if (o.idx != 0) continue;
        uint32_t times = 1u;
        if (keep) { const u64 ord = ((u64)o.ord_hi << 32) | o.ord_lo; times = (keep[ord] == 1 ? 1u : 0u) + (pcnt ? pcnt[ord] : 0u); }
        if (!times) continue;
        bool ok = true;
        for (int k = 0; k < o.nj; ++k) { const uint32_t s = occ[i + k].slot; if (s == 0xFFFFFFFFu || !acc2[s]) ok = false; }
        if (!ok) continue;
        for (int k = 0; k < o.nj; ++k) {
            const JbOcc q = occ[i + k];
            atomicAdd(&t.cnt2[q.slot], times);
            atomicMax(&t.le2[q.slot], (uint32_t)q.le);
            atomicMax(&t.re2[q.slot], (uint32_t)q.re);
        }
    }
}

struct JbOut { u64 key; uint32_t support, le, re; };
__global__ __launch_bounds__(256) void thj_k_jb_gather(JbTable t, const u64* sorted, int64_t n, JbOut* out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t s = jb_find(t.key, t.mask, sorted[i]);
        out[i] = JbOut{sorted[i], t.cnt2[s], t.le2[s], t.re2[s]};
    }
}

#include "thj_juncbed_fusion_impl.h"
#include "thj_juncbed_pair_impl.h"

// ------------------------------------------------------------------------------------------------ host side

static void jb_free(thj_ctx* c) {
    JbState& s = c->jb;
    for (JbStore* t : {&s.junc.tab, &s.indel.tab, &s.fus.tab}) t->release();
    s.junc.sorted.release(); s.junc.occ.release(); s.junc.known.release(); s.indel.occ.release();
    s.fus.grp.release(); s.fus.focc.release(); s.fus.uocc.release(); s.fus.jocc.release();
    s.best.rec.release(); s.best.skey.release(); s.best.keep.release(); s.best.cnt.release();
    s.acc.release(); s.um.release();
    s.pair.ins.release(); s.pair.pcnt.release(); s.pair.pprio.release(); s.pair.cnt.release();
    s = JbState{};
}

// `slots` slots for every table of the layout; a store that has them already stays as it is
static int jb_store_alloc(JbStore& s, const JbLayout& L, int64_t slots) {
    if (s.cap == slots) return THJ_OK;
    s.w64.release(); s.w32.release(); s.cap = 0; s.w64.cap = slots * L.tables * L.n64; s.w32.cap = slots * L.tables * L.n32;
    HIPCHK(hipMalloc(&s.w64.p, (size_t)s.w64.cap * sizeof(u64)));
    HIPCHK(hipMalloc(&s.w32.p, (size_t)s.w32.cap * sizeof(uint32_t)));
    if (!s.cnt.p) { HIPCHK(hipMalloc(&s.cnt.p, L.n_cnt * sizeof(unsigned long long))); s.cnt.cap = L.n_cnt; }
    s.cap = slots;
    return THJ_OK;
}
static int jb_store_reset(thj_ctx* c, const JbStore& s) {
    HIPCHK(hipMemsetAsync(s.w64.p, 0xFF, (size_t)s.w64.cap * sizeof(u64), c->stream));
    HIPCHK(hipMemsetAsync(s.w32.p, 0, (size_t)s.w32.cap * sizeof(uint32_t), c->stream));
    HIPCHK(hipMemsetAsync(s.cnt.p, 0, (size_t)s.cnt.cap * sizeof(unsigned long long), c->stream));
    return THJ_OK;
}
static u64* jb_col64(const JbStore& s, const JbLayout& L, int col, int table = 0) { return s.w64.p + ((size_t)table * L.n64 + col) * s.cap; }
static uint32_t* jb_col32(const JbStore& s, const JbLayout& L, int col, int table = 0) { return s.w32.p + ((size_t)table * L.n32 + col) * s.cap; }

static JbTable jb_table(thj_ctx* c) {
    const JbStore& s = c->jb.junc.tab;
    auto w = [&](int col) { return jb_col32(s, JB_LAYOUT, col); };
    return JbTable{jb_col64(s, JB_LAYOUT, JB_KEY), (u64)s.cap - 1, w(JB_CNT1), w(JB_LE1), w(JB_RE1), w(JB_CNT2), w(JB_LE2), w(JB_RE2), w(JB_LEFT), w(JB_ACC), w(JB_ACC2),
                   jb_col64(s, JB_LAYOUT, JB_LIST), s.cnt.p};
}
// which: 0 the deletion table, 1 the insertion table (only that one has priorities and letters)
static JbiTable jbi_table(thj_ctx* c, int which) {
    const JbStore& s = c->jb.indel.tab;
    auto u = [&](int col) { return jb_col64(s, JBI_LAYOUT, col, which); };
    auto w = [&](int col) { return jb_col32(s, JBI_LAYOUT, col, which); };
    return JbiTable{u(JBI_KEY), which ? u(JBI_PRIO) : nullptr, which ? u(JBI_BASES) : nullptr, u(JBI_LIST), (u64)s.cap - 1, w(JBI_CNT), w(JBI_LE), w(JBI_RE),
                    &s.cnt.p[JBI_DISTINCT_DEL + which], &s.cnt.p[JBI_OVERFLOW]};
}
static JbfTable jbf_table(thj_ctx* c) {
    const JbStore& s = c->jb.fus.tab;
    return JbfTable{jb_col64(s, JBF_LAYOUT, JBF_K0), jb_col64(s, JBF_LAYOUT, JBF_K1), jb_col32(s, JBF_LAYOUT, JBF_FID), jb_col32(s, JBF_LAYOUT, JBF_P1),
                    jb_col32(s, JBF_LAYOUT, JBF_LIST), (u64)s.cap - 1, s.cnt.p};
}
static Genome jb_genome(thj_ctx* c) { return Genome{c->d_blocks, c->d_contig_blk, c->d_contig_len, c->n_contigs}; }

static constexpr int JB_BLOCK = 256;           // the __launch_bounds__ of every kernel here
static dim3 jb_grid(int64_t n) { const int64_t b = (n + JB_BLOCK - 1) / JB_BLOCK; return dim3((unsigned)(b > 4096 ? 4096 : b)); }

static int jb_sort_keys(thj_ctx* c, const u64* in, u64* out, int64_t n) {
    return run_with_sort_tmp(c, [&](void* tmp, size_t& bytes) { return hipcub::DeviceRadixSort::SortKeys(tmp, bytes, in, out, n, 0, 64, c->stream); });
}
static int jb_sort_pairs(thj_ctx* c, const u64* k_in, u64* k_out, const uint32_t* v_in, uint32_t* v_out, int64_t n) {
    return run_with_sort_tmp(c, [&](void* tmp, size_t& bytes) { return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, k_in, k_out, v_in, v_out, n, 0, 64, c->stream); });
}

// scratch of one call: on every way out the stream idle first (a kernel or a copy may still be using it), then hipFree or the block cache
struct JbScratch {
    thj_ctx* c; bool cached; void* p = nullptr;
    explicit JbScratch(thj_ctx* c_, bool cached_ = false) : c(c_), cached(cached_) {}  JbScratch(const JbScratch&) = delete;
    ~JbScratch() { if (!p) return; (void)hipStreamSynchronize(c->stream); if (cached) thj_dev_release(c, p); else (void)hipFree(p); }
    int alloc(size_t bytes) { HIPCHK(hipMalloc(&p, bytes)); return THJ_OK; }
    template <class T> T* as() const { return (T*)p; }
};

// the slots all three tables get: twice the candidate set long_spanning_reads was given (its records cannot hold other junctions than
// those and the ones already in spliced segment hits), at least 2^20 slots, or what thj_juncbed_configure asked for; a power of two
static int jb_alloc(thj_ctx* c) {
    JbState::Junc& J = c->jb.junc;
    const int64_t want = c->jb.want > 0 ? c->jb.want : (c->n_span_junc * 4 > (1 << 20) ? c->n_span_junc * 4 : (1 << 20));
    int64_t p = 1 << 16;
    while (p < want) p <<= 1;
    if (p == J.tab.cap && J.sorted.p) return THJ_OK;
    J.sorted.release();
    if (const int rc = jb_store_alloc(J.tab, JB_LAYOUT, p)) return rc;
    HIPCHK(hipMalloc(&J.sorted.p, (size_t)p * sizeof(u64))); J.sorted.cap = p;
    return THJ_OK;
}

extern "C" int thj_juncbed_configure(thj_ctx* c, int64_t junction_capacity) {
    if (!c || junction_capacity < 1) { thj_set_error("thj_juncbed_configure: bad argument"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->jb.want = junction_capacity;
    return THJ_OK;
}

extern "C" int thj_juncbed_reset_async(thj_ctx* c) {
    if (!c) { thj_set_error("null ctx"); return THJ_EINVAL; }
    if (!c->d_blocks) { thj_set_error("no genome resident: call thj_genome_upload/adopt first"); return THJ_ESTATE; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    JbState& s = c->jb;
    if (const int rc = jb_alloc(c)) return rc;
    if (const int rc = jb_store_reset(c, s.junc.tab)) return rc;
    s.records = 0; s.junc.occ_used = 0; s.junc.rows.clear(); s.junc.n_known = 0; s.flt = jbk::ReadFilter{};
    s.indel.on = false; s.indel.occ_used = 0; s.indel.ins.clear(); s.indel.del.clear();
    s.fus.on = false; s.fus.groups = 0; s.fus.rows.clear();
    s.best.on = false; for (int64_t& x : s.best.counts) x = 0;
    s.acc.on = s.acc.chosen = s.acc.pairs = false; s.acc.calls.clear(); s.acc.replayed = 0; s.acc.replayed_records = 0; s.acc.pcalls.clear(); s.acc.p_nlr.clear();
    s.pair.on = false; s.pair.n_ins = s.pair.n_both = s.pair.n_cand = s.pair.n_big = s.pair.n_bigcand = 0; for (int64_t& x : s.pair.counts) x = 0;
    s.um.reset();
    return THJ_OK;
}

// what the calls between reset and the first add share: a junction table there, no record added yet
static int jb_collect_begin(thj_ctx* c, const char* who) {
    if (!c->jb.junc.tab.cap) { const int rc = thj_juncbed_reset_async(c); if (rc) return rc; }
    if (c->jb.records) { thj_set_error("%s: records were added already (call it between reset and the first add)", who); return THJ_ESTATE; }
    return THJ_OK;
}

extern "C" int thj_juncbed_collect_indels(thj_ctx* c, int32_t on) {
    if (!c) { thj_set_error("null ctx"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    if (const int rc = jb_collect_begin(c, "thj_juncbed_collect_indels")) return rc;
    // as many slots each as the junction table has
    if (on) { HIPCHK(hipStreamSynchronize(c->stream)); const int rc = jb_store_alloc(c->jb.indel.tab, JBI_LAYOUT, c->jb.junc.tab.cap); if (rc) return rc; }
    c->jb.indel.on = on != 0;
    return THJ_OK;
}

extern "C" int thj_juncbed_collect_fusions(thj_ctx* c, int32_t on, int32_t anchor_len, int32_t read_mismatches, int32_t multireads) {
    if (!c) { thj_set_error("null ctx"); return THJ_EINVAL; }
    if (on && (anchor_len < 0 || read_mismatches < 0 || multireads < 0)) { thj_set_error("thj_juncbed_collect_fusions: bad argument (anchor_len, read_mismatches, multireads >= 0)"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    if (const int rc = jb_collect_begin(c, "thj_juncbed_collect_fusions")) return rc;
    if (on && c->jb.pair.on) { thj_set_error("thj_juncbed_collect_fusions: inserts are being graded; the fusion set of the chosen pairs (pair_support) is not built"); return THJ_EINVAL; }
    if (on && c->jb.best.on) { thj_set_error("thj_juncbed_collect_fusions: best alignments are being chosen; the fusion set of the chosen alignments is not built"); return THJ_EINVAL; }
    JbState::Fus& F = c->jb.fus;
    F.on = false;
    if (!on) return THJ_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (const int rc = jb_store_alloc(F.tab, JBF_LAYOUT, c->jb.junc.tab.cap)) return rc;      // as many slots as the junction table has
    if (const int rc = jb_store_reset(c, F.tab)) return rc;
    F.anchor = anchor_len; F.mismatches = read_mismatches; F.multireads = multireads;
    F.groups = 0; F.rows.clear(); F.on = true;
    return THJ_OK;
}

// a list that grows keeps its first `keep` entries (the stream is idle); width: the buffer is that many arrays of cap entries, the first is kept
template <class T>
static int jb_grow(DevBuf<T>& b, unsigned long long keep, unsigned long long need, int width = 1) {
    if ((int64_t)need <= b.cap) return THJ_OK;
    const int64_t ncap = (int64_t)need + (int64_t)need / 4 + 4096;
    T* n = nullptr; HIPCHK(hipMalloc(&n, (size_t)ncap * width * sizeof(T)));
    if (b.p && keep) HIPCHK(hipMemcpy(n, b.p, (size_t)keep * sizeof(T), hipMemcpyDeviceToDevice));
    (void)hipFree(b.p); b.p = n; b.cap = ncap;
    return THJ_OK;
}

// The annotation: entries that can equal no junction of a record are dropped (jbk::known_entry_ok says which and why), the rest
// packed with junc_key, sorted and made unique on the device.  The array stays with the consensus state and grows like its lists.
extern "C" int thj_juncbed_known_junctions(thj_ctx* c, const thj_junction* juncs, int64_t n) {
    if (!c || n < 0 || (n > 0 && !juncs)) { thj_set_error("thj_juncbed_known_junctions: bad argument"); return THJ_EINVAL; }
    if (!c->d_blocks) { thj_set_error("no genome resident: call thj_genome_upload/adopt first"); return THJ_ESTATE; }
    HIPCHK(hipSetDevice(c->device));
    if (const int rc = jb_collect_begin(c, "thj_juncbed_known_junctions")) return rc;
    JbState::Junc& J = c->jb.junc;
    J.n_known = 0;
    const Genome g{nullptr, c->h_contig_blk.data(), nullptr, c->n_contigs};
    std::vector<u64> keys;
    keys.reserve((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const thj_junction& j = juncs[i];
        if (jbk::known_entry_ok(j.ref_id, j.left, j.right, c->n_contigs, c->h_lens.data())) keys.push_back(junc_key(g, j.ref_id, j.left, j.right, j.antisense != 0));
    }
    const int64_t m = (int64_t)keys.size();
    if (!m) return THJ_OK;
    if (m >= (1ll << 31)) { thj_set_error("thj_juncbed_known_junctions: more than 2^31 - 1 annotated junctions"); return THJ_EINVAL; }
    HIPCHK(hipStreamSynchronize(c->stream));
    if (const int rc = jb_grow(J.known, 0, (unsigned long long)m)) return rc;
    JbScratch tmp(c);                                           // [the keys as handed in | sorted | how many are distinct]
    if (const int rc = tmp.alloc((size_t)(2 * m + 1) * sizeof(u64))) return rc;
    u64 *d_in = tmp.as<u64>(), *d_sorted = d_in + m; unsigned long long* d_num = (unsigned long long*)(d_sorted + m);
    HIPCHK(hipMemcpyAsync(d_in, keys.data(), (size_t)m * sizeof(u64), hipMemcpyHostToDevice, c->stream));
    if (const int rc = jb_sort_keys(c, d_in, d_sorted, m)) return rc;
    if (const int rc = run_with_sort_tmp(c, [&](void* t, size_t& bytes) { return hipcub::DeviceSelect::Unique(t, bytes, (const u64*)d_sorted, J.known.p, d_num, (int)m, c->stream); })) return rc;
    unsigned long long distinct = 0;
    if (const int rc = read_device_value(c, (const unsigned long long*)d_num, &distinct)) return rc;
    J.n_known = (int64_t)distinct;
    return THJ_OK;
}

extern "C" int thj_juncbed_read_filter(thj_ctx* c, int32_t on, int32_t read_mismatches, int32_t read_gap_length, int32_t read_edit_dist) {
    if (!c) { thj_set_error("null ctx"); return THJ_EINVAL; }
    if (on && (read_mismatches < 0 || read_gap_length < 0 || read_edit_dist < 0)) { thj_set_error("thj_juncbed_read_filter: bad argument (read_mismatches, read_gap_length, read_edit_dist >= 0)"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    if (const int rc = jb_collect_begin(c, "thj_juncbed_read_filter")) return rc;
    c->jb.flt = on ? jbk::ReadFilter{1, read_mismatches, read_gap_length, read_edit_dist} : jbk::ReadFilter{};
    return THJ_OK;
}

extern "C" int thj_juncbed_best_alignments(thj_ctx* c, int32_t on, int32_t max_multihits, int32_t suppress_hits, int32_t bowtie2_max_penalty) {
    if (!c) { thj_set_error("null ctx"); return THJ_EINVAL; }
    if (on && (max_multihits < 1 || bowtie2_max_penalty < 0)) { thj_set_error("thj_juncbed_best_alignments: bad argument (max_multihits >= 1, bowtie2_max_penalty >= 0)"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    if (const int rc = jb_collect_begin(c, "thj_juncbed_best_alignments")) return rc;
    JbState::Best& B = c->jb.best;
    if (on && c->jb.fus.on) { thj_set_error("thj_juncbed_best_alignments: fusions are being collected; the fusion set of the chosen alignments is not built"); return THJ_EINVAL; }
    B.on = false; c->jb.pair.on = false; c->jb.um.on = false;  // (grading inserts, and collecting the unmapped reads, is asked for after this call, every time)
    if (!on) return THJ_OK;
    if (!B.cnt.p) { HIPCHK(hipMalloc(&B.cnt.p, JBB_N_COUNTERS * sizeof(unsigned long long))); B.cnt.cap = JBB_N_COUNTERS; }
    HIPCHK(hipMemsetAsync(B.cnt.p, 0, JBB_N_COUNTERS * sizeof(unsigned long long), c->stream));
    B.max_multihits = max_multihits; B.suppress = suppress_hits != 0; B.max_penalty = bowtie2_max_penalty; B.on = true;
    return THJ_OK;
}

// pairs: thj_juncbed_collect_accepted_pairs -- the same switch, and inserts may be graded beside it (thj_juncbed_report_pairs_bam writes their records)
static int jb_collect_accepted(thj_ctx* c, const char* who, bool pairs, int32_t on, int32_t library_type, const char* rg_id, const int32_t* tid_of_ref, int32_t n_ref) {
    if (!c) { thj_set_error("null ctx"); return THJ_EINVAL; }
    if (on && (n_ref < 0 || (n_ref > 0 && !tid_of_ref) || n_ref != c->n_contigs)) { thj_set_error("%s: bad argument (tid_of_ref names the output header's target of each of the genome's %d contigs)", who, (int)c->n_contigs); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    if (const int rc = jb_collect_begin(c, who)) return rc;
    JbState::Accepted& A = c->jb.acc;
    A.on = A.chosen = A.pairs = false; A.calls.clear(); A.replayed = 0; A.replayed_records = 0; A.pcalls.clear(); A.p_nlr.clear();
    if (!on) return THJ_OK;
    if (!c->jb.best.on) { thj_set_error("%s: best alignments are not being chosen (thj_juncbed_best_alignments first): the reported alignments are that choice", who); return THJ_ESTATE; }
    if (c->jb.pair.on && !pairs) { thj_set_error("thj_juncbed_collect_accepted: inserts are being graded; accepted hits for pairs (print_sam_for_pair) is not built by this switch (thj_juncbed_collect_accepted_pairs)"); return THJ_EINVAL; }
    A.library_type = library_type;
    A.rg.assign((const uint8_t*)(rg_id ? rg_id : ""), (const uint8_t*)(rg_id ? rg_id : "") + (rg_id ? strlen(rg_id) : 0));
    for (uint8_t ch : A.rg) if (ch == '\t') { thj_set_error("%s: a TAB in the read group id", who); return THJ_EINVAL; }
    A.tid.assign(tid_of_ref, tid_of_ref + n_ref); A.in_bytes = A.out_bytes = 0;
    A.on = true; A.pairs = pairs;
    return THJ_OK;
}
extern "C" int thj_juncbed_collect_accepted(thj_ctx* c, int32_t on, int32_t library_type, const char* rg_id, const int32_t* tid_of_ref, int32_t n_ref) {
    return jb_collect_accepted(c, "thj_juncbed_collect_accepted", false, on, library_type, rg_id, tid_of_ref, n_ref);
}
extern "C" int thj_juncbed_collect_accepted_pairs(thj_ctx* c, int32_t on, int32_t library_type, const char* rg_id, const int32_t* tid_of_ref, int32_t n_ref) {
    return jb_collect_accepted(c, "thj_juncbed_collect_accepted_pairs", true, on, library_type, rg_id, tid_of_ref, n_ref);
}

extern "C" int thj_juncbed_best_counts(thj_ctx* c, int64_t* counts) {
    if (!c || !counts) { thj_set_error("thj_juncbed_best_counts: bad argument"); return THJ_EINVAL; }
    for (int k = 0; k < 4; ++k) counts[k] = c->jb.best.counts[k];
    return THJ_OK;
}

extern "C" int thj_juncbed_pair_alignments(thj_ctx* c, int32_t on, int32_t inner_dist_mean, int32_t inner_dist_std_dev, int32_t fusion_min_dist, int32_t report_mixed,
                                           int32_t report_discordant) {
    if (!c) { thj_set_error("null ctx"); return THJ_EINVAL; }
    if (on && inner_dist_std_dev < 1) { thj_set_error("thj_juncbed_pair_alignments: bad argument (inner_dist_std_dev >= 1: the grade divides by it)"); return THJ_EINVAL; }
    if (on && fusion_min_dist < 0) { thj_set_error("thj_juncbed_pair_alignments: bad argument (fusion_min_dist >= 0)"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    if (const int rc = jb_collect_begin(c, "thj_juncbed_pair_alignments")) return rc;
    JbState& s = c->jb; JbState::Pair& P = s.pair;
    P.on = false;
    if (!on) return THJ_OK;
    if (!s.best.on) { thj_set_error("thj_juncbed_pair_alignments: best alignments are not being chosen (thj_juncbed_best_alignments first): grading inserts is that choice for pairs"); return THJ_ESTATE; }
    if (s.fus.on) { thj_set_error("thj_juncbed_pair_alignments: fusions are being collected; the fusion set of the chosen pairs (pair_support) is not built"); return THJ_EINVAL; }
    if (s.acc.on && !s.acc.pairs) { thj_set_error("thj_juncbed_pair_alignments: the reported alignments are being collected by thj_juncbed_collect_accepted; accepted hits for pairs (print_sam_for_pair) is not built by that switch (thj_juncbed_collect_accepted_pairs)"); return THJ_EINVAL; }
    if (!P.cnt.p) { HIPCHK(hipMalloc(&P.cnt.p, JBP_N_COUNTERS * sizeof(unsigned long long))); P.cnt.cap = JBP_N_COUNTERS; }
    P.mean = inner_dist_mean; P.sd = inner_dist_std_dev; P.fusion_min_dist = fusion_min_dist; P.mixed = report_mixed != 0; P.discordant = report_discordant != 0;
    P.n_ins = P.n_both = P.n_cand = P.n_big = P.n_bigcand = 0; for (int64_t& x : P.counts) x = 0;
    P.on = true;
    return THJ_OK;
}

extern "C" int thj_juncbed_pair_counts(thj_ctx* c, int64_t* counts) {
    if (!c || !counts) { thj_set_error("thj_juncbed_pair_counts: bad argument"); return THJ_EINVAL; }
    for (int k = 0; k < 5; ++k) counts[k] = c->jb.pair.counts[k];
    return THJ_OK;
}

static jbp::Cfg jbp_cfg(const JbState& s, bool final_report) {
    return jbp::Cfg{s.pair.mean, s.pair.sd, s.pair.fusion_min_dist, s.best.max_penalty, s.best.max_multihits, (uint8_t)s.pair.mixed, (uint8_t)s.pair.discordant, (uint8_t)(s.best.suppress ? 1 : 0),
                    (uint8_t)(final_report ? 1 : 0), s.um.on ? s.um.max_report_intron : 0};
}
// the lists thj_k_jbp_grade handed over (counters pc[JBP_BIG], pc[JBP_BIGCAND]): std::sort on every list's scores, the orders back at the same places
static int jbp_sort_big(thj_ctx* c, const unsigned long long* pc, const JbpBig* d_big, const int32_t* d_score, uint32_t* d_order) {
    unsigned long long h[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(h, pc + JBP_BIG, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (!h[0]) return THJ_OK;
    std::vector<JbpBig> big((size_t)h[0]); std::vector<int32_t> sc((size_t)h[1]); std::vector<uint32_t> ord((size_t)h[1]);
    HIPCHK(hipMemcpyAsync(big.data(), d_big, big.size() * sizeof(JbpBig), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(sc.data(), d_score, sc.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (const JbpBig& b : big) {
        if (b.off + b.n > h[1]) { thj_set_error("the lists of the inserts handed to the host for their sort do not add up"); return THJ_EINVAL; }
        jbp::sort_order(sc.data() + b.off, b.n, ord.data() + b.off);
    }
    HIPCHK(hipMemcpyAsync(d_order, ord.data(), ord.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                    // (the host vector was the copy's source)
    return THJ_OK;
}
// one block of scratch carved into 16-byte aligned pieces
struct JbpCarve {
    size_t total = 0; char* base = nullptr;
    size_t want(size_t bytes) { const size_t at = total; total += (bytes + 15) & ~(size_t)15; return at; }
    template <class T> T* at(size_t off) const { return (T*)(base + off); }
};

// an add call's two halves: the counters before, the count kernel, the counters after, the stream idle; grow(before, after) makes room in
// the lists (they are counted first, so that they are exactly large enough), add(before, after) launches the kernel that fills them
typedef const unsigned long long* JbCounts;
template <int N, class Count, class Grow, class Add>
static int jb_count_grow_add(thj_ctx* c, const unsigned long long* d_cnt, Count count, Grow grow, Add add) {
    unsigned long long before[N] = {}, after[N] = {};
    HIPCHK(hipMemcpyAsync(before, d_cnt, sizeof before, hipMemcpyDeviceToHost, c->stream));
    count();
    HIPCHK(hipMemcpyAsync(after, d_cnt, sizeof after, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (const int rc = grow(before, after)) return rc;
    return add(before, after);
}

// the fusion half of an add call, after the junction half: r's read_idx fields are below n_groups
static int jbf_add(thj_ctx* c, const JbRecs& r, int64_t n_groups) {
    JbState::Fus& F = c->jb.fus;
    const int64_t total = r.n_slots + r.n_extra;
    if (n_groups < 1) { thj_set_error("fusions are being collected: the add call knows no reads"); return THJ_EINVAL; }
    if (F.groups + n_groups > F.grp.cap) {                          // [group sizes | records of the group the filter drops]
        HIPCHK(hipStreamSynchronize(c->stream));
        if (const int rc = jb_grow(F.grp, F.groups, F.groups + n_groups, 2)) return rc;
    }
    uint32_t* grp1 = F.grp.p + F.groups;
    HIPCHK(hipMemsetAsync(grp1, 0, (size_t)n_groups * sizeof(uint32_t), c->stream));
    const Genome g = jb_genome(c);
    const JbfCfg cfg{F.anchor, F.mismatches, F.multireads};
    const JbfTable t = jbf_table(c);
    return jb_count_grow_add<JBF_N_COUNTERS>(c, t.cnt,
        [&] { hipLaunchKernelGGL(thj_k_jbf_count, jb_grid(total), dim3(JB_BLOCK), 0, c->stream, g, r, cfg, grp1, (u64)n_groups, t.cnt); },
        [&](JbCounts before, JbCounts after) {
            if (const int rc = jb_grow(F.focc, before[JBF_FOCC], after[JBF_FBOUND])) return rc;
            if (const int rc = jb_grow(F.uocc, before[JBF_UOCC], after[JBF_UBOUND])) return rc;
            return jb_grow(F.jocc, before[JBF_JOCC], after[JBF_JBOUND]);
        },
        [&](JbCounts, JbCounts) -> int {
            const u64 grp_base = (u64)F.groups; F.groups += n_groups;
            hipLaunchKernelGGL(thj_k_jbf_add, jb_grid(total), dim3(JB_BLOCK), 0, c->stream, g, r, jb_table(c), t, cfg, (const uint32_t*)grp1, (u64)n_groups, grp_base,
                               F.focc.p, (unsigned long long)F.focc.cap, F.uocc.p, (unsigned long long)F.uocc.cap, F.jocc.p, (unsigned long long)F.jocc.cap);
            HIPCHK(hipGetLastError());
            return THJ_OK;
        });
}

// n_groups: with fusions collected, the number of reads the records' read_idx fields count over
// mult, unflt: thj_juncbed_add_pairs' first pass (device arrays over the call's records; null from every other entry point, which
// inserts being graded refuses)
static int jb_add(thj_ctx* c, const JbRecs& recs, const JbiSeq& sq = JbiSeq{}, int64_t n_groups = 0, const uint32_t* mult = nullptr, const uint8_t* unflt = nullptr) {
    JbState& s = c->jb;
    if (!s.junc.tab.cap) { int rc = thj_juncbed_reset_async(c); if (rc) return rc; }
    if (s.pair.on && !mult) { thj_set_error("inserts are being graded (thj_juncbed_pair_alignments): the records of this consensus come through thj_juncbed_add_pairs"); return THJ_ESTATE; }
    JbRecs r = recs; r.flt = s.flt;                            // here the read filter reaches the count and add kernels of every entry point
    const int64_t total = r.n_slots + r.n_extra;
    if (total == 0) return THJ_OK;
    const bool indel = s.indel.on;
    if (s.records + total >= (1ll << 40)) { thj_set_error("more than 2^40 records in one consensus"); return THJ_EINVAL; }
    const JbTable t = jb_table(c);
    JbState::Best& B = s.best;
    if (B.on) {
        // ranks and pass-1 duplicates while the cigars are at hand: what is kept of record i of this call lies at B.rec[s.records + i]
        if (r.slot_layout || r.nrec || r.n_extra) { thj_set_error("best alignments are being chosen: the resident slot layout is not built (hand the records in as an array)"); return THJ_EINVAL; }
        HIPCHK(hipStreamSynchronize(c->stream));
        if (const int e = jb_grow(B.rec, (unsigned long long)s.records, (unsigned long long)(s.records + total))) return e;
        hipLaunchKernelGGL(thj_k_jbb_rank, jb_grid(total), dim3(JB_BLOCK), 0, c->stream, r, B.rec.p + s.records, B.cnt.p);
        HIPCHK(hipGetLastError());
    }
    r.unflt = unflt;                                           // (the ranks above are made without it: such a record competes in neither pass)
    const int rc = jb_count_grow_add<JB_N_COUNTERS>(c, t.counters,
        [&] { hipLaunchKernelGGL(indel ? thj_k_jb_count<true> : thj_k_jb_count<false>, jb_grid(total), dim3(JB_BLOCK), 0, c->stream, r, t.counters); },
        [&](JbCounts before, JbCounts after) {
            int e = jb_grow(s.junc.occ, before[JB_OCC_COUNTED], after[JB_OCC_COUNTED]);
            if (!e && B.on) e = jb_grow(B.skey, before[JB_OCC_COUNTED], after[JB_OCC_COUNTED]);
            return e || !indel ? e : jb_grow(s.indel.occ, before[JB_IOCC_COUNTED], after[JB_IOCC_COUNTED]);
        },
        [&](JbCounts before, JbCounts after) -> int {
            const u64 ord_base = (u64)s.records; s.records += total;
            if (after[JB_OCC_COUNTED] == before[JB_OCC_COUNTED] && after[JB_IOCC_COUNTED] == before[JB_IOCC_COUNTED]) return THJ_OK;
            // (without INDEL the kernel does not look at the indel list)
            hipLaunchKernelGGL(indel ? thj_k_jb_add<true> : thj_k_jb_add<false>, jb_grid(total), dim3(JB_BLOCK), 0, c->stream, jb_genome(c), r, t,
                               s.junc.occ.p, (unsigned long long)(B.on && B.skey.cap < s.junc.occ.cap ? B.skey.cap : s.junc.occ.cap), sq, s.indel.occ.p,
                               (unsigned long long)s.indel.occ.cap, ord_base, B.on ? B.rec.p + ord_base : (JbbRec*)nullptr, B.skey.p, mult);
            HIPCHK(hipGetLastError());
            s.junc.occ_used = (int64_t)after[JB_OCC_COUNTED]; s.indel.occ_used = (int64_t)after[JB_IOCC_COUNTED];
            return THJ_OK;
        });
    if (rc) return rc;
    return s.fus.on ? jbf_add(c, r, n_groups) : THJ_OK;
}

extern "C" int thj_juncbed_add_span_async(thj_ctx* c) {
    if (!c) { thj_set_error("null ctx"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    if (c->jb.indel.on) { thj_set_error("thj_juncbed_add_span_async: indels are being collected, the records' bases are needed (thj_juncbed_add_span_seq_async)"); return THJ_EINVAL; }
    if (c->jb.best.on) { thj_set_error("thj_juncbed_add_span_async: best alignments are being chosen; choosing among the resident records of a pass is not built"); return THJ_EINVAL; }
    JbRecs r{(const OutAln*)c->d_aln_pool, c->d_nrec, c->span_reads, (const OutAln*)c->d_aln_sorted, c->n_ovf, true};
    return jb_add(c, r, JbiSeq{}, c->span_reads);
}

extern "C" int thj_juncbed_add_span_seq_async(thj_ctx* c, const thj_span_batch* batch) {
    if (!c || !batch) { thj_set_error("thj_juncbed_add_span_seq_async: bad argument"); return THJ_EINVAL; }
    if (!c->jb.indel.on) return thj_juncbed_add_span_async(c);
    if (c->jb.best.on) { thj_set_error("thj_juncbed_add_span_seq_async: best alignments are being chosen; choosing among the resident records of a pass is not built"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->n_alns == 0) return THJ_OK;
    if (!batch->read_planes || !batch->read_len || batch->words_per_plane < 1) { thj_set_error("thj_juncbed_add_span_seq_async: the batch holds no reads"); return THJ_EINVAL; }
    // the records in thj_span_download's order: that order says which of two insertions is the first
    JbScratch alns(c, true);
    const int rc = thj_span_compact_device(c, &alns.p);
    if (rc == THJ_EFALLBACK) { thj_set_error("thj_juncbed_add_span_seq_async: the pass's records could not be put in order on the device"); return THJ_EFALLBACK; }
    if (rc) return rc;
    JbRecs r{alns.as<const OutAln>(), nullptr, c->n_alns, nullptr, 0, false};
    JbiSeq sq{nullptr, nullptr, (const u64*)batch->read_planes, batch->read_len, batch->words_per_plane, batch->n_reads};
    return jb_add(c, r, sq, c->span_reads);
}

// ref_id, n_cigar and -- for a fusion alignment -- ref_id2 of host records, before anything is launched
static int jb_check_records(thj_ctx* c, const thj_aln* recs, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (recs[i].ref_id < 1 || (int32_t)recs[i].ref_id > c->n_contigs || recs[i].n_cigar > 16) { thj_set_error("record %lld: contig or cigar out of range", (long long)i); return THJ_EINVAL; }
    if (c->jb.best.on)
        for (int64_t i = 0; i < n; ++i) {
            if ((int64_t)recs[i].read_idx >= n) { thj_set_error("record %lld: read_idx %u, but the call has %lld records (best alignments are being chosen: read_idx numbers the reads of the call from 0)", (long long)i, recs[i].read_idx, (long long)n); return THJ_EINVAL; }
            if (i && recs[i].read_idx < recs[i - 1].read_idx) { thj_set_error("record %lld: read_idx %u after %u (best alignments are being chosen: a read's records follow each other and read_idx does not fall)", (long long)i, recs[i].read_idx, recs[i - 1].read_idx); return THJ_EINVAL; }
        }
    if (c->jb.fus.on)
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
    JbScratch tmp(c), d_off(c), d_bases(c);
    if (const int rc = tmp.alloc((size_t)n * sizeof(thj_aln))) return rc;
    HIPCHK(hipMemcpyAsync(tmp.p, recs, (size_t)n * sizeof(thj_aln), hipMemcpyHostToDevice, c->stream));
    JbiSeq sq{};
    if (ins_off) {
        const size_t nb = (size_t)ins_off[n];
        if (const int rc = d_off.alloc((size_t)(n + 1) * 8)) return rc;
        if (const int rc = d_bases.alloc(nb + 16)) return rc;
        HIPCHK(hipMemcpyAsync(d_off.p, ins_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, c->stream));
        if (nb) HIPCHK(hipMemcpyAsync(d_bases.p, ins_bases, nb, hipMemcpyHostToDevice, c->stream));
        sq.ins_off = d_off.as<const int64_t>(); sq.ins_bases = d_bases.as<const uint8_t>();
    }
    JbRecs r{tmp.as<const OutAln>(), nullptr, n, nullptr, 0, false};
    return jb_add(c, r, sq, n);
}

// the unmapped reads are being collected: the reads of a host-array call (runs under one read_idx) wait for thj_juncbed_read_numbers
static void jb_um_added_host(thj_ctx* c, const thj_aln* recs, int64_t n) {
    if (!c->jb.um.on) return;
    std::vector<uint32_t> runs;
    for (int64_t i = 0; i < n; ++i) { if (i && recs[i].read_idx == recs[i - 1].read_idx) ++runs.back(); else runs.push_back(1u); }
    thj_um_added(c, (int64_t)runs.size(), false, runs.data(), (int64_t)runs.size(), 0);
}

extern "C" int thj_juncbed_add_records(thj_ctx* c, const thj_aln* recs, int64_t n, int32_t on_device) {
    if (!c || n < 0 || (n > 0 && !recs)) { thj_set_error("thj_juncbed_add_records: bad argument"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    if (n == 0) return THJ_OK;
    if (on_device && c->jb.um.on) { thj_set_error("thj_juncbed_add_records: the unmapped reads are being collected; device arrays beside it are not built (their reads cannot be numbered)"); return THJ_EINVAL; }
    if (on_device) { JbRecs r{(const OutAln*)recs, nullptr, n, nullptr, 0, false}; return jb_add(c, r, JbiSeq{}, n); }
    if (const int rc = thj_um_add_ok(c, "thj_juncbed_add_records")) return rc;
    if (const int rc = jb_check_records(c, recs, n)) return rc;
    if (c->jb.indel.on)
        for (int64_t i = 0; i < n; ++i)
            if (jbw::inss(recs[i].cigar, recs[i].n_cigar, recs[i].left, recs[i].ref_id, [](uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, int) {})) {
                thj_set_error("thj_juncbed_add_records: record %lld has an insertion and indels are being collected: its bases are needed (thj_juncbed_add_records_seq)", (long long)i);
                return THJ_EINVAL;
            }
    if (const int rc = jb_add_host(c, recs, n, nullptr, nullptr)) return rc;
    jb_um_added_host(c, recs, n);
    return THJ_OK;
}

// the letters handed in beside host records (ins_off, ins_bases as thj_juncbed_add_records_seq takes them): everything is looked at before
// anything is counted
static int jb_check_seq(thj_ctx* c, const char* who, const thj_aln* recs, int64_t n, const int64_t* ins_off, const char* ins_bases) {
    if (ins_off[0] != 0 || (ins_off[n] > 0 && !ins_bases)) { thj_set_error("%s: bad argument (ins_off[0] must be 0)", who); return THJ_EINVAL; }
    for (int64_t i = 0; i < n; ++i) {
        int64_t at = ins_off[i]; bool bad_ref = false; uint32_t too_long = 0;
        if (ins_off[i + 1] < at) { thj_set_error("%s: ins_off falls at record %lld", who, (long long)i); return THJ_EINVAL; }
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
    return THJ_OK;
}

extern "C" int thj_juncbed_add_records_seq(thj_ctx* c, const thj_aln* recs, int64_t n, const int64_t* ins_off, const char* ins_bases) {
    if (!c || n < 0 || (n > 0 && (!recs || !ins_off))) { thj_set_error("thj_juncbed_add_records_seq: bad argument"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    if (n == 0) return THJ_OK;
    if (const int rc = thj_um_add_ok(c, "thj_juncbed_add_records_seq")) return rc;
    if (const int rc = jb_check_records(c, recs, n)) return rc;
    if (const int rc = jb_check_seq(c, "thj_juncbed_add_records_seq", recs, n, ins_off, ins_bases)) return rc;
    if (const int rc = jb_add_host(c, recs, n, ins_off, (const uint8_t*)ins_bases)) return rc;
    jb_um_added_host(c, recs, n);
    return THJ_OK;
}

// The left and the right reads of a run of inserts: merged by number into the reference's visit order (tophat_reports.cpp:2002-2097 -- the
// smaller number goes first as a singleton, equal numbers are an insert: its left records, then its right records), every side a read of
// its own for the single-end kernels; the first pass of the inserts (thj_k_jbp_grade, thj_k_jbp_settle_first) before the records are counted.
// off / bases [0] left, [1] right: the inserted letters per side (thj_juncbed_add_pairs_seq), or null
static int jbp_add_pairs(thj_ctx* c, const thj_aln* left, int64_t n_left, const thj_aln* right, int64_t n_right, const int64_t* const* off, const char* const* bases) {
    HIPCHK(hipSetDevice(c->device));
    JbState& s = c->jb; JbState::Pair& P = s.pair;
    if (!P.on) { thj_set_error("thj_juncbed_add_pairs: inserts are not being graded (thj_juncbed_pair_alignments first)"); return THJ_ESTATE; }
    const int64_t n = n_left + n_right;
    if (n == 0) return THJ_OK;
    if (const int rc = thj_um_add_ok(c, "thj_juncbed_add_pairs")) return rc;
    if (s.records + n >= (1ll << 31)) { thj_set_error("thj_juncbed_add_pairs: more than 2^31 - 1 records with best alignments chosen"); return THJ_EINVAL; }
    // everything is looked at before anything is counted
    for (int side = 0; side < 2; ++side) {
        const thj_aln* r = side ? right : left; const int64_t m = side ? n_right : n_left; const char* name = side ? "right" : "left";
        for (int64_t i = 0; i < m; ++i) {
            if (r[i].ref_id < 1 || (int32_t)r[i].ref_id > c->n_contigs || r[i].n_cigar > 16) { thj_set_error("%s record %lld: contig or cigar out of range", name, (long long)i); return THJ_EINVAL; }
            if ((int64_t)r[i].read_idx >= n) { thj_set_error("%s record %lld: read_idx %u, but the call has %lld records (read_idx numbers the inserts of the call from 0)", name, (long long)i, r[i].read_idx, (long long)n); return THJ_EINVAL; }
            if (i && r[i].read_idx < r[i - 1].read_idx) { thj_set_error("%s record %lld: read_idx %u after %u (an insert's records follow each other and read_idx does not fall within a side)", name, (long long)i, r[i].read_idx, r[i - 1].read_idx); return THJ_EINVAL; }
            if (s.indel.on && !off && jbw::inss(r[i].cigar, r[i].n_cigar, r[i].left, r[i].ref_id, [](uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, int) {})) {
                thj_set_error("thj_juncbed_add_pairs: %s record %lld has an insertion and indels are being collected: its bases are needed (thj_juncbed_add_pairs_seq)", name, (long long)i);
                return THJ_EINVAL;
            }
        }
        if (off && m) { const int rc = jb_check_seq(c, "thj_juncbed_add_pairs_seq", r, m, off[side], bases[side]); if (rc) return rc; }
    }
    std::vector<int64_t> m_off; std::string m_bases;           // the letters in the merged order
    if (off) { m_off.reserve((size_t)n + 1); m_off.push_back(0); }
    auto letters = [&](int side, int64_t i) {
        if (!off) return;
        const int64_t len = off[side][i + 1] - off[side][i];
        if (len > 0) m_bases.append(bases[side] + off[side][i], (size_t)len);
        m_off.push_back((int64_t)m_bases.size());
    };
    std::vector<thj_aln> recs; recs.reserve((size_t)n);
    std::vector<JbpIns> groups;
    std::vector<uint32_t> mult; mult.reserve((size_t)n);
    const u64 cap = 2ull * (u64)s.best.max_multihits + 1ull;
    int64_t n_both = 0, call_cand = 0, call_big = 0, call_bigcand = 0;
    uint32_t side_no = 0;                                       // every side is a read of its own for the per-record kernels
    for (int64_t i = 0, j = 0; i < n_left || j < n_right;) {
        const u64 li = i < n_left ? left[i].read_idx : ~0ull, rj = j < n_right ? right[j].read_idx : ~0ull, id = li < rj ? li : rj;
        JbpIns g{(u64)s.records + recs.size(), (u64)(P.n_cand + call_cand), 0u, 0u};
        if (li == id) { for (; i < n_left && left[i].read_idx == id; ++i, ++g.nl) { recs.push_back(left[i]); recs.back().read_idx = side_no; letters(0, i); } ++side_no; }
        if (rj == id) { for (; j < n_right && right[j].read_idx == id; ++j, ++g.nr) { recs.push_back(right[j]); recs.back().read_idx = side_no; letters(1, j); } ++side_no; }
        const bool both = g.nl && g.nr;
        mult.insert(mult.end(), (size_t)(g.nl + g.nr), both ? 0u : JBP_SINGLE_END);
        if (both) {
            const u64 prod = (g.nl < cap ? g.nl : cap) * (g.nr < cap ? g.nr : cap);
            ++n_both; call_cand += (int64_t)prod;
            if (prod > jbp::SORT_SMALL) { ++call_big; call_bigcand += (int64_t)prod; }
        }
        groups.push_back(g);
    }
    const int64_t ng = (int64_t)groups.size();
    HIPCHK(hipStreamSynchronize(c->stream));
    if (const int rc = jb_grow(P.ins, (unsigned long long)P.n_ins, (unsigned long long)(P.n_ins + ng))) return rc;
    JbpCarve cv;
    const size_t o_rec = cv.want((size_t)n * sizeof(thj_aln)), o_mult = cv.want((size_t)n * 4), o_unflt = cv.want((size_t)n), o_cand = cv.want((size_t)call_cand * sizeof(JbpCand)),
                 o_nk = cv.want((size_t)ng * 4), o_fl = cv.want((size_t)ng * 4), o_gbig = cv.want((size_t)ng * 8), o_big = cv.want((size_t)call_big * sizeof(JbpBig)),
                 o_sc = cv.want((size_t)call_bigcand * 4), o_ord = cv.want((size_t)call_bigcand * 4), o_ioff = cv.want(off ? (size_t)(n + 1) * 8 : 0),
                 o_ibases = cv.want(off ? m_bases.size() + 16 : 0);
    JbScratch tmp(c);
    if (const int rc = tmp.alloc(cv.total + 16)) return rc;
    cv.base = tmp.as<char>();
    JbpIns* d_ins = P.ins.p + P.n_ins;
    HIPCHK(hipMemcpyAsync(cv.at<thj_aln>(o_rec), recs.data(), (size_t)n * sizeof(thj_aln), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(cv.at<uint32_t>(o_mult), mult.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_ins, groups.data(), (size_t)ng * sizeof(JbpIns), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(cv.at<uint8_t>(o_unflt), 0, (size_t)n, c->stream));
    JbiSeq sq{};
    if (off) {
        HIPCHK(hipMemcpyAsync(cv.at<int64_t>(o_ioff), m_off.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, c->stream));
        if (!m_bases.empty()) HIPCHK(hipMemcpyAsync(cv.at<char>(o_ibases), m_bases.data(), m_bases.size(), hipMemcpyHostToDevice, c->stream));
        sq.ins_off = cv.at<const int64_t>(o_ioff); sq.ins_bases = cv.at<const uint8_t>(o_ibases);
    }
    JbRecs r{cv.at<const OutAln>(o_rec), nullptr, n, nullptr, 0, false};
    if (n_both) {
        HIPCHK(hipMemsetAsync(P.cnt.p + JBP_BIG, 0, 2 * sizeof(unsigned long long), c->stream));
        JbRecs rf = r; rf.flt = s.flt;
        const JbpSrcFirst src{rf, s.records};
        const u64 cand_base = (u64)P.n_cand;
        hipLaunchKernelGGL(thj_k_jbp_grade<JbpSrcFirst>, jb_grid(ng), dim3(JB_BLOCK), 0, c->stream, src, jb_genome(c), JbpResc{nullptr, 0}, jbp_cfg(s, false), (const JbpIns*)d_ins, ng, cand_base,
                           cv.at<JbpCand>(o_cand), cv.at<uint32_t>(o_nk), cv.at<uint32_t>(o_fl), cv.at<u64>(o_gbig), cv.at<JbpBig>(o_big), (unsigned long long)call_big,
                           cv.at<int32_t>(o_sc), (unsigned long long)call_bigcand, P.cnt.p);
        HIPCHK(hipGetLastError());
        if (call_big) { const int rc = jbp_sort_big(c, P.cnt.p, cv.at<JbpBig>(o_big), cv.at<int32_t>(o_sc), cv.at<uint32_t>(o_ord)); if (rc) return rc; }
        hipLaunchKernelGGL(thj_k_jbp_settle_first, jb_grid(ng), dim3(JB_BLOCK), 0, c->stream, src, (const JbpIns*)d_ins, ng, cand_base, cv.at<const JbpCand>(o_cand),
                           cv.at<const uint32_t>(o_nk), cv.at<const u64>(o_gbig), cv.at<const uint32_t>(o_ord), cv.at<uint32_t>(o_mult), cv.at<uint8_t>(o_unflt));
        HIPCHK(hipGetLastError());
    }
    if (const int rc = jb_add(c, r, sq, n, cv.at<const uint32_t>(o_mult), cv.at<const uint8_t>(o_unflt))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));                    // (the host vectors were the copies' sources)
    if (s.acc.on) {                                             // thj_juncbed_report_pairs_bam replays exactly this call
        s.acc.pcalls.push_back(JbState::Accepted::PCall{n_left, n_right, s.records - n, P.n_ins, ng});
        for (const JbpIns& g : groups) { s.acc.p_nlr.push_back(g.nl); s.acc.p_nlr.push_back(g.nr); }
    }
    P.n_ins += ng; P.n_both += n_both; P.n_cand += call_cand; P.n_big += call_big; P.n_bigcand += call_bigcand;
    if (s.um.on) {                                              // the call's inserts wait for thj_juncbed_read_numbers
        int64_t has_l = 0, has_r = 0;
        for (const JbpIns& g : groups) { has_l += g.nl != 0u; has_r += g.nr != 0u; }
        thj_um_added(c, ng, false, nullptr, has_l, has_r);
    }
    return THJ_OK;
}

extern "C" int thj_juncbed_add_pairs(thj_ctx* c, const thj_aln* left, int64_t n_left, const thj_aln* right, int64_t n_right) {
    if (!c || n_left < 0 || n_right < 0 || (n_left > 0 && !left) || (n_right > 0 && !right)) { thj_set_error("thj_juncbed_add_pairs: bad argument"); return THJ_EINVAL; }
    return jbp_add_pairs(c, left, n_left, right, n_right, nullptr, nullptr);
}
extern "C" int thj_juncbed_add_pairs_seq(thj_ctx* c, const thj_aln* left, int64_t n_left, const int64_t* left_ins_off, const char* left_ins_bases, const thj_aln* right, int64_t n_right,
                                         const int64_t* right_ins_off, const char* right_ins_bases) {
    if (!c || n_left < 0 || n_right < 0 || (n_left > 0 && (!left || !left_ins_off)) || (n_right > 0 && (!right || !right_ins_off))) { thj_set_error("thj_juncbed_add_pairs_seq: bad argument"); return THJ_EINVAL; }
    const int64_t* off[2] = {left_ins_off, right_ins_off}; const char* bases[2] = {left_ins_bases, right_ins_bases};
    return jbp_add_pairs(c, left, n_left, right, n_right, off, bases);
}

// A piece (whole BGZF members) of a BAM of reported alignments: inflated, parsed, put in file order and numbered by read on the device
// (thj_ingest_reported, thj_ingest.hip), then added as device records.  Nothing is counted unless the whole piece can be.
extern "C" int thj_juncbed_add_bam(thj_ctx* c, const thj_bam_piece* piece, int32_t max_report_intron, int32_t more_follows, int64_t* n_records,
                                   uint32_t* resume_member, uint32_t* resume_skip) {
    if (!c || !piece || piece->comp_bytes < 0 || (piece->comp_bytes > 0 && !piece->comp) || piece->n_tid < 0 || (piece->n_tid > 0 && !piece->tid2ref) || !n_records ||
        !resume_member || !resume_skip) { thj_set_error("thj_juncbed_add_bam: bad argument"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    *n_records = 0; *resume_member = 0; *resume_skip = 0;
    if (!c->jb.junc.tab.cap) { const int rc = thj_juncbed_reset_async(c); if (rc) return rc; }
    if (!c->d_contig_names || c->n_contig_names != c->n_contigs) {
        thj_set_error("thj_juncbed_add_bam: the context holds no names for the genome's %d contigs (thj_bam_contig_names_upload): a fusion alignment names its contigs", (int)c->n_contigs);
        return THJ_ESTATE;
    }
    for (int32_t t = 0; t < piece->n_tid; ++t)
        if ((int64_t)piece->tid2ref[t] > (int64_t)c->n_contigs) { thj_set_error("thj_juncbed_add_bam: tid2ref[%d] = %u, the genome has %d contigs", (int)t, piece->tid2ref[t], (int)c->n_contigs); return THJ_EINVAL; }
    if (const int rc = thj_um_add_ok(c, "thj_juncbed_add_bam")) return rc;
    thj_reported_recs r;
    if (const int rc = thj_ingest_reported(c, piece, max_report_intron, c->jb.indel.on, c->jb.fus.on, c->jb.best.on, more_follows, &r)) return rc;
    JbScratch bases(c, true);
    bases.p = r.ins_bases;
    *resume_member = r.resume_member; *resume_skip = r.resume_skip;
    if (r.n == 0) return THJ_OK;
    if (c->jb.um.on && !c->jb.pair.on) { if (const int rc = thj_um_numbers_bam(c, &r)) { *resume_member = 0; *resume_skip = 0; return rc; } }
    const JbRecs recs{(const OutAln*)r.recs, nullptr, r.n, nullptr, 0, false};
    JbiSeq sq{};
    if (c->jb.indel.on) { sq.ins_off = r.ins_off; sq.ins_bases = r.ins_bases; }
    if (const int rc = jb_add(c, recs, sq, r.n_groups)) return rc;
    if (c->jb.acc.on) c->jb.acc.calls.push_back(r.n);          // thj_juncbed_report_bam replays exactly these
    if (c->jb.um.on) thj_um_added(c, r.n_groups, true, nullptr, r.n_groups, 0);
    *n_records = r.n;
    return THJ_OK;
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
    JbState::Indel& I = c->jb.indel; const JbState::Junc& J = c->jb.junc;
    I.ins.clear(); I.del.clear();
    if (!I.on) return THJ_OK;
    if (const int rc = jb_store_reset(c, I.tab)) return rc;
    const JbiTable td = jbi_table(c, 0), ti = jbi_table(c, 1);
    const uint8_t* keep = c->jb.best.on ? (const uint8_t*)c->jb.best.keep.p : nullptr;
    const uint32_t *pcnt = c->jb.pair.on ? (const uint32_t*)c->jb.pair.pcnt.p : nullptr, *pprio = c->jb.pair.on ? (const uint32_t*)c->jb.pair.pprio.p : nullptr;
    if (I.occ_used) {
        hipLaunchKernelGGL(thj_k_jbi_second, jb_grid(I.occ_used), dim3(JB_BLOCK), 0, c->stream, td, ti, (const JbiOcc*)I.occ.p, I.occ_used, (const JbOcc*)J.occ.p, J.occ_used,
                           (const uint32_t*)jb_table(c).acc2, keep, pcnt, pprio);
        hipLaunchKernelGGL(thj_k_jbi_letters, jb_grid(I.occ_used), dim3(JB_BLOCK), 0, c->stream, ti, (const JbiOcc*)I.occ.p, I.occ_used, keep, pcnt, pprio);
        HIPCHK(hipGetLastError());
    }
    unsigned long long h[JBI_N_COUNTERS];
    HIPCHK(hipMemcpyAsync(h, I.tab.cnt.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int64_t room = I.tab.cap - I.tab.cap / 4;
    if (h[JBI_OVERFLOW] || (int64_t)h[JBI_DISTINCT_DEL] > room || (int64_t)h[JBI_DISTINCT_INS] > room) {
        thj_set_error("indel table full (%llu distinct deletions, %llu distinct insertions, capacity %lld each): call thj_juncbed_configure with a larger capacity and add the records again",
                      h[JBI_DISTINCT_DEL], h[JBI_DISTINCT_INS], (long long)I.tab.cap);
        return THJ_EOVERFLOW;
    }
    for (int which = 0; which < 2; ++which) {
        const int64_t n = (int64_t)h[JBI_DISTINCT_DEL + which];
        if (!n) continue;
        const JbiTable t = which ? ti : td;
        if (const int rc = jb_sort_keys(c, t.list, J.sorted.p, n)) return rc;
        JbScratch d_out(c);
        if (const int rc = d_out.alloc((size_t)n * sizeof(JbiOut))) return rc;
        hipLaunchKernelGGL(thj_k_jbi_gather, jb_grid(n), dim3(JB_BLOCK), 0, c->stream, t, (const u64*)J.sorted.p, n, d_out.as<JbiOut>());
        std::vector<JbiOut> out((size_t)n);
        HIPCHK(hipMemcpyAsync(out.data(), d_out.p, (size_t)n * sizeof(JbiOut), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (auto& o : out) {
            uint32_t ref_id, left;
            jb_locate(c, o.key >> 30, &ref_id, &left);
            if (which) {
                thj_insstat s; memset(&s, 0, sizeof s);
                s.ref_id = ref_id; s.left = left; s.len = (uint32_t)(o.key & 0xFFu); s.support = o.support; s.left_extent = o.le; s.right_extent = o.re;
                for (uint32_t k = 0; k < s.len && k < (uint32_t)JBI_MAX_INS; ++k) s.bases[k] = "ACGTN???"[(o.bases >> (3 * k)) & 7u];
                I.ins.push_back(s);
            } else {
                thj_juncstat s;
                s.ref_id = ref_id; s.left = left; s.right = left + (uint32_t)((o.key >> 1) & ((1ull << 29) - 1)); s.antisense = 0;
                s.left_extent = o.le; s.right_extent = o.re; s.support = o.support; s.reserved = 0;
                I.del.push_back(s);
            }
        }
    }
    return THJ_OK;
}

// the fusion half of finish, after acc2 is known: drops, pass 2, the pass-1 set's ends, unsupport, rows
static int jbf_finish(thj_ctx* c) {
    JbState::Fus& F = c->jb.fus;
    F.rows.clear();
    if (!F.on) return THJ_OK;
    const JbfTable t = jbf_table(c);
    unsigned long long h[JBF_N_COUNTERS];
    HIPCHK(hipMemcpyAsync(h, t.cnt, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (h[JBF_FLAGS]) { thj_set_error("thj_juncbed_finish: the fusions of the records added cannot be counted: a record points outside the reads of its add call or outside the genome"); return THJ_EINVAL; }
    if (h[JBF_OVERFLOW] || (int64_t)h[JBF_DISTINCT] > F.tab.cap - F.tab.cap / 4) {
        thj_set_error("fusion table full (%llu distinct fusions, capacity %lld): call thj_juncbed_configure with a larger capacity and add the records again", h[JBF_DISTINCT], (long long)F.tab.cap);
        return THJ_EOVERFLOW;
    }
    const int64_t n_f = (int64_t)h[JBF_DISTINCT], n_focc = (int64_t)h[JBF_FOCC], n_uocc = (int64_t)h[JBF_UOCC], n_jocc = (int64_t)h[JBF_JOCC];
    if (!n_f) return THJ_OK;
    const uint32_t *grp1 = F.grp.p, *acc2 = jb_table(c).acc2; uint32_t* gdrop = F.grp.p + F.grp.cap;
    // one block of scratch: statistics, rows, the ends and their sorted copy
    const size_t b_st = ((size_t)n_f * sizeof(JbfStat) + 15) & ~(size_t)15, b_out = ((size_t)n_f * sizeof(thj_fusstat) + 15) & ~(size_t)15, b_key = (size_t)n_f * 2 * 8, b_val = (size_t)n_f * 2 * 4;
    JbScratch scratch(c);
    if (const int rc = scratch.alloc(b_st + b_out + 2 * b_key + 2 * b_val)) return rc;
    char* d = scratch.as<char>();
    JbfStat* st = (JbfStat*)d; thj_fusstat* out = (thj_fusstat*)(d + b_st);
    u64 *k_in = (u64*)(d + b_st + b_out), *k_out = k_in + n_f * 2; uint32_t *v_in = (uint32_t*)(k_out + n_f * 2), *v_out = v_in + n_f * 2;
    HIPCHK(hipMemsetAsync(st, 0, b_st, c->stream));
    HIPCHK(hipMemsetAsync(gdrop, 0, (size_t)F.groups * sizeof(uint32_t), c->stream));
    HIPCHK(hipMemsetAsync(&t.cnt[JBF_ENDS], 0, sizeof(unsigned long long), c->stream));
    if (n_jocc) hipLaunchKernelGGL(thj_k_jbf_drop, jb_grid(n_jocc), dim3(JB_BLOCK), 0, c->stream, F.jocc.p, n_jocc, acc2, gdrop);
    if (n_focc) hipLaunchKernelGGL(thj_k_jbf_second, jb_grid(n_focc), dim3(JB_BLOCK), 0, c->stream, t, (const JbfOcc*)F.focc.p, n_focc, (const JbfJOcc*)F.jocc.p, n_jocc,
                                   grp1, (const uint32_t*)gdrop, (int)F.multireads, st);
    hipLaunchKernelGGL(thj_k_jbf_ends, jb_grid(n_f), dim3(JB_BLOCK), 0, c->stream, t, n_f, k_in, v_in);
    unsigned long long n_ends = 0;
    HIPCHK(hipMemcpyAsync(&n_ends, &t.cnt[JBF_ENDS], sizeof n_ends, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (n_ends && n_uocc) {
        if (const int rc = jb_sort_pairs(c, k_in, k_out, v_in, v_out, (int64_t)n_ends)) return rc;
        hipLaunchKernelGGL(thj_k_jbf_unsupport, jb_grid(n_uocc), dim3(JB_BLOCK), 0, c->stream, (const JbfUOcc*)F.uocc.p, n_uocc, grp1, (const uint32_t*)gdrop,
                           (int)F.multireads, (const u64*)k_out, (const uint32_t*)v_out, (int64_t)n_ends, st);
    }
    hipLaunchKernelGGL(thj_k_jbf_gather, dim3((unsigned)(n_f > 4096 ? 4096 : n_f)), dim3(JB_BLOCK), 0, c->stream, jb_genome(c), t, (const JbfStat*)st, n_f, out);      // a workgroup per fusion
    HIPCHK(hipGetLastError());
    std::vector<thj_fusstat> rows((size_t)n_f);
    HIPCHK(hipMemcpyAsync(rows.data(), out, (size_t)n_f * sizeof(thj_fusstat), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (auto& r : rows) {
        if (!r.count) continue;                                                           // print_fusions: count > 0 only
        if (!n_ends) {
            // an empty pass-1 set: the reference's second pass then runs like its first (update_stat = fusions_ref.size() > 0,
            // tophat_reports.cpp:1167) and only counts
            r.unsupport = r.left_ext = r.right_ext = r.n_diffs = 0;
            memset(r.diffs, 0, sizeof r.diffs); memset(r.left_bases, 0, sizeof r.left_bases); memset(r.right_bases, 0, sizeof r.right_bases);
            memset(r.seq1, 0, sizeof r.seq1); memset(r.seq2, 0, sizeof r.seq2);
        }
        F.rows.push_back(r);
    }
    std::sort(F.rows.begin(), F.rows.end(), [](const thj_fusstat& a, const thj_fusstat& b) {      // Fusion::operator<, fusions.h:39-67
        return std::make_tuple(a.ref_id1, a.ref_id2, a.left, a.right, a.dir) < std::make_tuple(b.ref_id1, b.ref_id2, b.left, b.right, b.dir);
    });
    return THJ_OK;
}

// The second pass of the inserts, after thj_k_jbb_score: what it leaves on the device until the choice is through.
struct JbpFinal {
    JbScratch mem; const int32_t* score = nullptr; int32_t* score1 = nullptr; JbpCand* cand = nullptr; uint32_t *gnk = nullptr, *gflags = nullptr, *order = nullptr; u64* gbig = nullptr;
    explicit JbpFinal(thj_ctx* c) : mem(c) {}
};
static int jbp_second(thj_ctx* c, JbpFinal& f, int64_t n_juncs, const int32_t* score, JbbOver* over, int64_t over_cap) {
    JbState& s = c->jb; JbState::Best& B = s.best; JbState::Pair& P = s.pair;
    const int64_t n = s.records, ng = P.n_ins;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (P.pcnt.cap < n) { if (const int e = jb_grow(P.pcnt, 0, (unsigned long long)n)) return e; }
    if (P.pprio.cap < n) { if (const int e = jb_grow(P.pprio, 0, (unsigned long long)n)) return e; }
    if (s.um.on) { if (const int e = jb_grow(s.um.iword, 0, (unsigned long long)ng + 1)) return e; }
    // the reported alignments are written out afterwards: the lists stay with the context instead of going back with the scratch
    JbState::Accepted& A = s.acc;
    const bool stay = A.on;
    JbpCarve cv;
    const size_t o_s1 = cv.want((size_t)n * 4), o_cand = cv.want(stay ? 0 : (size_t)P.n_cand * sizeof(JbpCand)), o_nk = cv.want(stay ? 0 : (size_t)ng * 4), o_fl = cv.want(stay ? 0 : (size_t)ng * 4),
                 o_gbig = cv.want(stay ? 0 : (size_t)ng * 8), o_big = cv.want((size_t)P.n_big * sizeof(JbpBig)), o_sc = cv.want((size_t)P.n_bigcand * 4), o_ord = cv.want(stay ? 0 : (size_t)P.n_bigcand * 4),
                 o_flag = cv.want((size_t)n_juncs), o_keys = cv.want((size_t)n_juncs * 8), o_num = cv.want(8);
    if (const int rc = f.mem.alloc(cv.total + 16)) return rc;
    cv.base = f.mem.as<char>();
    f.score = score; f.score1 = cv.at<int32_t>(o_s1); f.cand = cv.at<JbpCand>(o_cand); f.gnk = cv.at<uint32_t>(o_nk); f.gflags = cv.at<uint32_t>(o_fl); f.gbig = cv.at<u64>(o_gbig);
    f.order = cv.at<uint32_t>(o_ord);
    if (stay) {
        if (const int e = jb_grow(A.p_cand, 0, (unsigned long long)P.n_cand + 1)) return e;
        if (const int e = jb_grow(A.p_gnk, 0, (unsigned long long)ng + 1)) return e;
        if (const int e = jb_grow(A.p_gflags, 0, (unsigned long long)ng + 1)) return e;
        if (const int e = jb_grow(A.p_gbig, 0, (unsigned long long)ng + 1)) return e;
        if (const int e = jb_grow(A.p_mword, 0, (unsigned long long)ng + 1)) return e;
        if (const int e = jb_grow(A.p_order, 0, (unsigned long long)P.n_bigcand + 1)) return e;
        f.cand = A.p_cand.p; f.gnk = A.p_gnk.p; f.gflags = A.p_gflags.p; f.gbig = A.p_gbig.p; f.order = A.p_order.p;
        HIPCHK(hipMemsetAsync(A.p_mword.p, 0xFF, ((size_t)ng + 1) * sizeof(uint32_t), c->stream));
    }
    HIPCHK(hipMemsetAsync(P.pcnt.p, 0, (size_t)n * sizeof(uint32_t), c->stream));
    HIPCHK(hipMemsetAsync(P.pprio.p, 0xFF, (size_t)n * sizeof(uint32_t), c->stream));
    HIPCHK(hipMemsetAsync(P.cnt.p, 0, JBP_N_COUNTERS * sizeof(unsigned long long), c->stream));
    // a record of no group (there is none: every record came through thj_juncbed_add_pairs) would keep its score
    HIPCHK(hipMemcpyAsync(f.score1, score, (size_t)n * 4, hipMemcpyDeviceToDevice, c->stream));
    if (!ng) return THJ_OK;
    // the first-pass junctions of support >= 10, still in sorted order
    JbpResc rs{nullptr, 0};
    if (n_juncs > 0) {
        const JbTable t = jb_table(c);
        hipLaunchKernelGGL(thj_k_jbp_resc_flags, jb_grid(n_juncs), dim3(JB_BLOCK), 0, c->stream, t, (const u64*)s.junc.sorted.p, n_juncs, cv.at<uint8_t>(o_flag));
        HIPCHK(hipGetLastError());
        if (const int rc = run_with_sort_tmp(c, [&](void* tmp, size_t& bytes) {
                return hipcub::DeviceSelect::Flagged(tmp, bytes, (const u64*)s.junc.sorted.p, cv.at<const uint8_t>(o_flag), cv.at<u64>(o_keys), cv.at<unsigned long long>(o_num), (int)n_juncs, c->stream);
            })) return rc;
        unsigned long long n_resc = 0;
        if (const int rc = read_device_value(c, (const unsigned long long*)cv.at<unsigned long long>(o_num), &n_resc)) return rc;
        rs = JbpResc{cv.at<const u64>(o_keys), (int64_t)n_resc};
    }
    const JbpSrcFinal src{B.rec.p, score};
    const jbp::Cfg cfg = jbp_cfg(s, true);
    hipLaunchKernelGGL(thj_k_jbp_grade<JbpSrcFinal>, jb_grid(ng), dim3(JB_BLOCK), 0, c->stream, src, jb_genome(c), rs, cfg, (const JbpIns*)P.ins.p, ng, (u64)0, f.cand, f.gnk, f.gflags, f.gbig,
                       cv.at<JbpBig>(o_big), (unsigned long long)P.n_big, cv.at<int32_t>(o_sc), (unsigned long long)P.n_bigcand, P.cnt.p);
    HIPCHK(hipGetLastError());
    if (P.n_big) { const int rc = jbp_sort_big(c, P.cnt.p, cv.at<JbpBig>(o_big), cv.at<int32_t>(o_sc), f.order); if (rc) return rc; }
    hipLaunchKernelGGL(thj_k_jbp_settle, jb_grid(ng), dim3(JB_BLOCK), 0, c->stream, src, cfg, (const JbpIns*)P.ins.p, ng, (const JbpCand*)f.cand, (const uint32_t*)f.gnk, f.gflags,
                       (const u64*)f.gbig, (const uint32_t*)f.order, f.score1, P.pcnt.p, P.pprio.p, over, (unsigned long long)over_cap, &B.cnt.p[JBB_LISTED], P.cnt.p,
                       s.um.on ? s.um.iword.p : (uint32_t*)nullptr);
    HIPCHK(hipGetLastError());
    unsigned long long h[JBP_N_COUNTERS];
    HIPCHK(hipMemcpyAsync(h, P.cnt.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 5; ++k) P.counts[k] = (int64_t)h[k];
    return THJ_OK;
}

// the choice among every read's alignments, after acc2 is known: B.keep[ordinal] = 1 for the
// records that are reported.  Reads over the cap: the device lists them, the host walks them in input order with the generator.
// n_juncs: the distinct junctions of the first pass, sorted in junc.sorted (the too_far rescue of the pair grade searches them)
static int jbb_choose(thj_ctx* c, int64_t n_juncs) {
    JbState& s = c->jb; JbState::Best& B = s.best; JbState::Pair& P = s.pair;
    const int64_t n = s.records;
    for (int64_t& x : B.counts) x = 0;
    for (int64_t& x : P.counts) x = 0;
    if (!n) { if (s.acc.on) { s.acc.h_draw.clear(); s.acc.chosen = true; s.acc.replayed = 0; s.acc.replayed_records = 0; } return THJ_OK; }
    if (n >= (1ll << 31)) { thj_set_error("thj_juncbed_finish: more than 2^31 - 1 records with best alignments chosen"); return THJ_EINVAL; }
    if (B.keep.cap < n) { HIPCHK(hipStreamSynchronize(c->stream)); if (const int e = jb_grow(B.keep, 0, (unsigned long long)n)) return e; }
    // scratch: scores, the reporting flags and their running sums, the list of reads over the cap (at most one read in max_multihits + 1 records)
    const int64_t over_cap = n / ((int64_t)B.max_multihits + 1) + 1 + (P.on ? P.n_both : 0);
    const size_t b_i32 = (((size_t)n + 1) * 4 + 15) & ~(size_t)15;
    JbScratch scratch(c);
    if (const int rc = scratch.alloc(3 * b_i32 + (size_t)over_cap * sizeof(JbbOver))) return rc;
    char* d = scratch.as<char>();
    int32_t* score = (int32_t*)d; uint32_t *reports = (uint32_t*)(d + b_i32), *before = (uint32_t*)(d + 2 * b_i32); JbbOver* over = (JbbOver*)(d + 3 * b_i32);
    // the reported alignments are written out afterwards: the scores and the reporting reads before every record stay with the context
    JbState::Accepted& A = s.acc;
    A.chosen = false;
    if (A.on) {
        HIPCHK(hipStreamSynchronize(c->stream));
        if (const int e = jb_grow(A.score, 0, (unsigned long long)n)) return e;
        if (const int e = jb_grow(A.before, 0, (unsigned long long)n + 1)) return e;
        score = A.score.p; before = A.before.p;
    }
    // the unmapped reads are written out afterwards: read_best_alignments' code of every read stays with the context
    uint8_t* code = nullptr;
    if (s.um.on) {
        HIPCHK(hipStreamSynchronize(c->stream));
        if (const int e = jb_grow(s.um.code, 0, (unsigned long long)n)) return e;
        code = s.um.code.p;
        HIPCHK(hipMemsetAsync(code, 0, (size_t)n, c->stream));
    }
    HIPCHK(hipMemsetAsync(reports + n, 0, 4, c->stream));
    HIPCHK(hipMemsetAsync(&B.cnt.p[JBB_READS], 0, 3 * sizeof(unsigned long long), c->stream));
    HIPCHK(hipMemsetAsync(&B.cnt.p[JBB_LISTED], 0, sizeof(unsigned long long), c->stream));
    const JbTable t = jb_table(c);
    hipLaunchKernelGGL(thj_k_jbb_score, jb_grid(n), dim3(JB_BLOCK), 0, c->stream, t, (const JbbRec*)B.rec.p, n, (const JbOcc*)s.junc.occ.p, s.junc.occ_used,
                       (const u64*)B.skey.p, (const uint32_t*)t.acc2, (const u64*)s.junc.known.p, s.junc.n_known, (int)B.max_penalty, score);
    // inserts are graded: their lists first; what is left for the single-end way competes under score1
    JbpFinal pf(c);
    if (P.on) { const int rc = jbp_second(c, pf, n_juncs, score, over, over_cap); if (rc) return rc; score = pf.score1; }
    hipLaunchKernelGGL(thj_k_jbb_choose, jb_grid(n), dim3(JB_BLOCK), 0, c->stream, (const JbbRec*)B.rec.p, n, (const int32_t*)score, B.keep.p);
    hipLaunchKernelGGL(thj_k_jbb_cap, jb_grid(n), dim3(JB_BLOCK), 0, c->stream, (const JbbRec*)B.rec.p, n, B.keep.p, (uint32_t)B.max_multihits, (int)B.suppress, reports,
                       over, (unsigned long long)over_cap, B.cnt.p, code);
    if (P.on && P.n_ins) hipLaunchKernelGGL(thj_k_jbp_reports, jb_grid(P.n_ins), dim3(JB_BLOCK), 0, c->stream, (const JbpIns*)P.ins.p, P.n_ins, (const uint32_t*)pf.gflags, reports);
    HIPCHK(hipGetLastError());
    unsigned long long h[JBB_N_COUNTERS];
    HIPCHK(hipMemcpyAsync(h, B.cnt.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    B.counts[0] = (int64_t)h[JBB_READS]; B.counts[1] = (int64_t)h[JBB_LOST]; B.counts[2] = (int64_t)h[JBB_OVER]; B.counts[3] = (int64_t)h[JBB_DUPS];
    const int64_t n_over = (int64_t)h[JBB_LISTED];
    if (!n_over && !A.on) return THJ_OK;                         // no read is over the cap (or --suppress-hits): nothing is generated
    if (n_over > over_cap) { thj_set_error("thj_juncbed_finish: more reads over the cap than records allow"); return THJ_EINVAL; }
    if (const int rc = run_with_sort_tmp(c, [&](void* tmp, size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, (const uint32_t*)reports, before, (int)n + 1, c->stream); })) return rc;
    uint32_t n_reporting = 0;                                    // reads of which anything is reported: one print_sam_for_single draw each
    if (A.on) { if (const int rc = read_device_value(c, (const uint32_t*)before + n, &n_reporting)) return rc; A.h_draw.assign((size_t)n_reporting, 0u); }
    uint32_t* kept = A.on ? A.h_draw.data() : nullptr;
    std::vector<JbbOver> list((size_t)n_over);
    if (n_over) {
        hipLaunchKernelGGL(thj_k_jbb_before, jb_grid(n_over), dim3(JB_BLOCK), 0, c->stream, over, n_over, (const uint32_t*)before);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(list.data(), over, (size_t)n_over * sizeof(JbbOver), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    std::sort(list.begin(), list.end(), [](const JbbOver& a, const JbbOver& b) { return a.first < b.first || (a.first == b.first && a.pad && !b.pad); });      // input order (an insert before its left read)
    std::vector<uint32_t> mask;
    std::vector<uint8_t> alive;
    jbb::CapWalk walk;
    walk.begin();
    u64 seen = 0;                                               // reporting reads the generator has passed
    for (JbbOver& o : list) {
        if (o.pad) {                                            // an insert over the cap: the draws among its ties, then print_sam_for_pair's
            const uint32_t better = (o.pad & ~JBP_GIVEN_UP) - 1u, ties = o.n;
            if (kept) { if (o.before > n_reporting) { thj_set_error("thj_juncbed_finish: the reads over the cap and the reporting reads do not add up"); return THJ_EINVAL; }
                        walk.rest(o.before - seen, kept + seen); }
            else walk.rng.discard(o.before - seen);
            alive.assign(ties, 1);
            jbp::trim_pairs(better, ties, (uint32_t)B.max_multihits, [&walk]() { return walk.rng.next(); }, alive.data());
            seen = o.before;
            if (o.pad & JBP_GIVEN_UP) continue;                 // (mixed alignments: its sides follow as single reads, at the same record)
            const uint32_t own = walk.rng.next();                // print_sam_for_pair's draw: the primary pair (kept on request)
            if (kept) { if (o.before >= n_reporting) { thj_set_error("thj_juncbed_finish: the reads over the cap and the reporting reads do not add up"); return THJ_EINVAL; }
                        kept[o.before] = own; }
            seen = o.before + 1;
            o.word = (uint32_t)mask.size();
            mask.resize(mask.size() + (o.left + 31) / 32, 0u);
            for (uint32_t k = 0; k < better + ties && k < o.left; ++k) if (k < better || alive[k - better]) mask[o.word + (k >> 5)] |= 1u << (k & 31u);
            continue;
        }
        alive.assign(o.left, 1);
        walk.read(o.before - seen, o.left, (uint32_t)B.max_multihits, alive.data(), kept ? kept + seen : nullptr);
        seen = o.before + 1;
        o.word = (uint32_t)mask.size();
        mask.resize(mask.size() + (o.left + 31) / 32, 0u);
        for (uint32_t k = 0; k < o.left; ++k) if (alive[k]) mask[o.word + (k >> 5)] |= 1u << (k & 31u);
        if (mask.size() >= (1ull << 31)) { thj_set_error("thj_juncbed_finish: more than 2^36 alignments of reads over the cap"); return THJ_EINVAL; }
    }
    if (A.on) {
        if (seen > n_reporting) { thj_set_error("thj_juncbed_finish: the reads over the cap and the reporting reads do not add up"); return THJ_EINVAL; }
        walk.rest(n_reporting - seen, kept + seen);
        if (const int e = jb_grow(A.draw, 0, (unsigned long long)n_reporting + 1)) return e;
        if (n_reporting) HIPCHK(hipMemcpyAsync(A.draw.p, A.h_draw.data(), (size_t)n_reporting * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        A.chosen = true; A.replayed = 0; A.replayed_records = 0;
    }
    if (!n_over) { HIPCHK(hipStreamSynchronize(c->stream)); return THJ_OK; }
    JbScratch d_mask(c);
    if (const int rc = d_mask.alloc(mask.size() * sizeof(uint32_t))) return rc;
    HIPCHK(hipMemcpyAsync(over, list.data(), (size_t)n_over * sizeof(JbbOver), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_mask.p, mask.data(), mask.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    uint32_t* mword = nullptr;                                  // the masks of the inserts over the cap stay as well
    if (A.on && P.on) {
        if (const int e = jb_grow(A.p_mask, 0, (unsigned long long)mask.size() + 1)) return e;
        HIPCHK(hipMemcpyAsync(A.p_mask.p, mask.data(), mask.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        mword = A.p_mword.p;
    }
    const int64_t blocks = (n_over + 3) / 4;
    hipLaunchKernelGGL(thj_k_jbb_trim, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(JB_BLOCK), 0, c->stream, (const JbbRec*)B.rec.p, B.keep.p, (const JbbOver*)over, n_over,
                       d_mask.as<const uint32_t>());
    if (P.on) hipLaunchKernelGGL(thj_k_jbp_apply, jb_grid(n_over), dim3(JB_BLOCK), 0, c->stream, JbpSrcFinal{B.rec.p, pf.score}, (const JbpIns*)P.ins.p, P.n_ins, (const JbpCand*)pf.cand,
                                 (const uint32_t*)pf.gnk, (const u64*)pf.gbig, (const uint32_t*)pf.order, (const JbbOver*)over, n_over, d_mask.as<const uint32_t>(), P.pcnt.p, P.pprio.p, mword);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));                    // (the host vectors were the copies' sources)
    return THJ_OK;
}

// the junction half of finish, n > 0 distinct junctions: filters (acc2), second pass, final set
static int jb_finish_juncs(thj_ctx* c, int64_t n, int32_t min_anchor_len) {
    JbState::Junc& J = c->jb.junc;
    const JbTable t = jb_table(c);
    hipLaunchKernelGGL(thj_k_jb_accept, jb_grid(J.tab.cap), dim3(JB_BLOCK), 0, c->stream, t, n, (int)min_anchor_len, (const u64*)J.known.p, J.n_known);
    if (const int rc = jb_sort_keys(c, t.list, J.sorted.p, n)) return rc;
    hipLaunchKernelGGL(thj_k_jb_knockout, jb_grid(n), dim3(JB_BLOCK), 0, c->stream, t, (const u64*)J.sorted.p, n, (int)min_anchor_len, t.acc2, J.n_known > 0);
    // second pass (cnt2 / le2 / re2, the columns from JB_CNT2 up to JB_LEFT, start from zero: a finish can be repeated)
    if (c->jb.best.on) { const int rc = jbb_choose(c, n); if (rc) return rc; }
    HIPCHK(hipMemsetAsync(t.cnt2, 0, (size_t)J.tab.cap * (JB_LEFT - JB_CNT2) * sizeof(uint32_t), c->stream));
    if (J.occ_used) hipLaunchKernelGGL(thj_k_jb_second, jb_grid(J.occ_used), dim3(JB_BLOCK), 0, c->stream, t, (const JbOcc*)J.occ.p, J.occ_used, (const uint32_t*)t.acc2,
                                       c->jb.best.on ? (const uint8_t*)c->jb.best.keep.p : (const uint8_t*)nullptr,
                                       c->jb.pair.on ? (const uint32_t*)c->jb.pair.pcnt.p : (const uint32_t*)nullptr);
    JbScratch d_out(c);
    if (const int rc = d_out.alloc((size_t)n * sizeof(JbOut))) return rc;
    hipLaunchKernelGGL(thj_k_jb_gather, jb_grid(n), dim3(JB_BLOCK), 0, c->stream, t, (const u64*)J.sorted.p, n, d_out.as<JbOut>());
    HIPCHK(hipGetLastError());
    std::vector<JbOut> out((size_t)n);
    HIPCHK(hipMemcpyAsync(out.data(), d_out.p, (size_t)n * sizeof(JbOut), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (auto& o : out) {
        if (o.support == 0 || o.le < 8 || o.re < 8) continue;                          // tophat_reports.cpp:2974-2984
        thj_juncstat s;
        jb_locate(c, o.key >> 30, &s.ref_id, &s.left);
        s.right = s.left + (uint32_t)((o.key >> 1) & ((1ull << 29) - 1)); s.antisense = (uint32_t)(o.key & 1ull);
        s.left_extent = o.le; s.right_extent = o.re; s.support = o.support; s.reserved = 0;
        J.rows.push_back(s);
    }
    return THJ_OK;
}

extern "C" int thj_juncbed_finish(thj_ctx* c, int32_t min_anchor_len, int64_t* n_juncs) {
    if (!c || min_anchor_len < 0 || min_anchor_len > 60) { thj_set_error("thj_juncbed_finish: bad argument (min_anchor_len 0..60)"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    JbState& s = c->jb;
    s.junc.rows.clear(); s.indel.ins.clear(); s.indel.del.clear(); s.fus.rows.clear(); if (n_juncs) *n_juncs = 0;
    s.um.chosen = false;
    if (!s.junc.tab.cap) return THJ_OK;
    unsigned long long h[JB_N_COUNTERS];
    HIPCHK(hipMemcpyAsync(h, s.junc.tab.cnt.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (h[JB_OVERFLOW] || (int64_t)h[JB_DISTINCT] > s.junc.tab.cap - s.junc.tab.cap / 4) {
        thj_set_error("junction table full (%llu distinct junctions, capacity %lld): call thj_juncbed_configure with a larger capacity and add the records again",
                      h[JB_DISTINCT], (long long)s.junc.tab.cap);
        return THJ_EOVERFLOW;
    }
    if (s.indel.on && h[JB_IFLAGS]) {
        thj_set_error("thj_juncbed_finish: the indels of the records added cannot be counted:%s%s%s",
                      h[JB_IFLAGS] & JBI_FLAG_LONG ? " an insertion is longer than the 16 bases that are held;" : "",
                      h[JB_IFLAGS] & JBI_FLAG_RANGE ? " a record points outside the genome, its batch or its bases;" : "",
                      h[JB_IFLAGS] & JBI_FLAG_NOSEQ ? " a record with an insertion came without bases;" : "");
        return THJ_EINVAL;
    }
    const int64_t n = (int64_t)h[JB_DISTINCT];
    if (n) { const int rc = jb_finish_juncs(c, n, min_anchor_len); if (rc) return rc; }
    else if (s.best.on) { const int rc = jbb_choose(c, 0); if (rc) return rc; }           // (no junction was ever seen: the scores are the records' own)
    if (const int rc = jbi_finish(c)) { s.junc.rows.clear(); return rc; }
    if (const int rc = jbf_finish(c)) { s.junc.rows.clear(); s.indel.ins.clear(); s.indel.del.clear(); return rc; }
    if (n_juncs) *n_juncs = (int64_t)s.junc.rows.size();
    if (s.um.on) { s.um.chosen = true; s.um.replay(); }       // thj_juncbed_report_unmapped_bam may begin
    return THJ_OK;
}

template <class T> static void jb_copy_rows(const std::vector<T>& rows, T* out) { if (!rows.empty()) memcpy(out, rows.data(), rows.size() * sizeof(T)); }
extern "C" int thj_juncbed_download(thj_ctx* c, thj_juncstat* out) {
    if (!c || (!c->jb.junc.rows.empty() && !out)) { thj_set_error("thj_juncbed_download: bad argument"); return THJ_EINVAL; }
    jb_copy_rows(c->jb.junc.rows, out);
    return THJ_OK;
}

extern "C" int thj_juncbed_indel_counts(thj_ctx* c, int64_t* n_ins, int64_t* n_del) {
    if (!c) { thj_set_error("null ctx"); return THJ_EINVAL; }
    if (n_ins) *n_ins = (int64_t)c->jb.indel.ins.size();
    if (n_del) *n_del = (int64_t)c->jb.indel.del.size();
    return THJ_OK;
}

extern "C" int thj_juncbed_indel_download(thj_ctx* c, thj_insstat* ins, thj_juncstat* dels) {
    if (!c || (!c->jb.indel.ins.empty() && !ins) || (!c->jb.indel.del.empty() && !dels)) { thj_set_error("thj_juncbed_indel_download: bad argument"); return THJ_EINVAL; }
    jb_copy_rows(c->jb.indel.ins, ins); jb_copy_rows(c->jb.indel.del, dels);
    return THJ_OK;
}

extern "C" int thj_juncbed_fusion_count(thj_ctx* c, int64_t* n) {
    if (!c) { thj_set_error("null ctx"); return THJ_EINVAL; }
    if (n) *n = (int64_t)c->jb.fus.rows.size();
    return THJ_OK;
}

extern "C" int thj_juncbed_fusion_download(thj_ctx* c, thj_fusstat* out) {
    if (!c || (!c->jb.fus.rows.empty() && !out)) { thj_set_error("thj_juncbed_fusion_download: bad argument"); return THJ_EINVAL; }
    jb_copy_rows(c->jb.fus.rows, out);
    return THJ_OK;
}

// accepted_hits.bam for graded inserts: the output records of the lists the finish kept (thj_juncbed_report_pairs_bam, thj_accepted.hip)
#include "thj_accepted_pair_impl.h"
