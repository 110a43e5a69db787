// thj_juncbed_best_impl.h -- which alignments of a read count: read_best_alignments in both of its modes, the AlignStatus score and the
// --max-multihits cap, beside the junction consensus (included by thj_juncbed_impl.h; the decisions themselves: thj_best_core.h).
// Single-end: every read is a singleton (tophat_reports.cpp:2006-2023, :2229-2322).
//
// A read = the records of one add call that follow each other under one read_idx.  Every kernel here gives a record a lane; a lane finds
// its read by walking to the neighbours that share it and counts over the read's records (the ones below its own: its rank), so a read
// of one record and a read of hundreds take the same path, a read may lie across waves, workgroups and grid strides, and no group size is
// refused.  Lanes next to each other read the same records of a large read: those loads are broadcasts.
//
// At add time, while the cigars are at hand (thj_k_jbb_rank): the rank under BowtieHit::operator< and the first pass's std::unique -- a
// record equal (cmp_read_equal) to the one before it in rank order is no record for thj_k_jb_add's first-pass atomics; its occurrences are
// still listed -- and the 40 bytes kept of every record until finish.  thj_k_jb_add adds where the record's junction occurrences start
// and, per occurrence, the key AlignStatus will ask about (its own walk: always the first contig).
// At finish, after acc2 is known: thj_k_jbb_score (exclusion and score per record), thj_k_jbb_choose (maximum, ties, the second unique
// in rank order -> a keep flag per record), thj_k_jbb_cap (what is left per read; reads over --max-multihits are listed).  The host walks
// that list in input order with the generator (jbb::CapWalk) and thj_k_jbb_trim clears the flags of the alignments it erases.
// thj_k_jb_second, thj_k_jbi_second (and through it the letters pass) read the keep flags.
#pragma once
#include "thj_best_core.h"
#include "thj_jbb_rec.h"
#include "thj_unmapped_core.h"

static constexpr int32_t JBB_OUT = INT32_MIN;                 // the score of a record that does not compete (filtered or excluded)
static constexpr u64 JBB_NO_KEY = ~0ull;                      // a junction that can be in no set (it lies outside its contig)
enum { JBB_READS, JBB_LOST, JBB_OVER, JBB_DUPS, JBB_LISTED, JBB_N_COUNTERS = 8 };
struct JbbOver { u64 first; uint32_t n, left; u64 before; uint32_t word, pad; };     // a read over the cap: records [first, first + n), `left` kept; reporting reads before it; its bits in the mask

__device__ __forceinline__ jbb::Key jbb_key_of(const OutAln& a) {
    const JbCigar cg{(const uint32_t*)&a, false};
    return jbb::key_of(a.ref_id, a.left, (a.flags & 1u) != 0, a.mismatches, a.n_cigar < SPAN_MAXC ? a.n_cigar : SPAN_MAXC, cg);
}
__device__ __forceinline__ jbb::Key jbb_key_of(const JbbRec& r) {
    jbb::Key k; k.ref_id = r.ref_id; k.ref_id2 = r.ref_id2; k.left = r.left; k.right = r.right; k.anti = (r.flags & JBB_ANTI) ? 1 : 0;
    k.mismatches = r.mismatches; k.edit_dist = r.edit_dist; k.n_cigar = r.n_cigar;
    return k;
}
// the key AlignStatus looks up: contig `ref`, or none when junc_key could not hold it (it would fold onto another junction's key)
__device__ __forceinline__ u64 jbb_score_key(const Genome& g, uint32_t ref, uint32_t left, uint32_t right, bool anti) {
    const uint32_t span = right - left; const int64_t l = (int64_t)(int32_t)left;
    if (ref < 1u || ref > (uint32_t)g.n_contigs || span < 1u || span > (uint32_t)jbk::SPAN_MASK || l < -1 || l >= (int64_t)g.contig_len[ref - 1]) return JBB_NO_KEY;
    return junc_key(g, ref, left, right, anti);
}

// records of a plain array (r.slots[0 .. r.n_slots)); out[i] = what is kept of record i
__global__ __launch_bounds__(256) void thj_k_jbb_rank(JbRecs r, JbbRec* out, unsigned long long* counters) {
    const int64_t total = r.n_slots;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t rd = r.slots[i].read_idx;
        int64_t s = i, e = i + 1;
        while (s > 0 && r.slots[s - 1].read_idx == rd) --s;
        while (e < total && r.slots[e].read_idx == rd) ++e;
        const OutAln* a = jb_rec(r, i);
        JbbRec o{};
        o.flags = (uint8_t)((i == s ? JBB_FIRST : 0) | (a ? 0 : JBB_GONE));
        if (a) {
            const JbCigar ca{(const uint32_t*)a, false};
            const jbb::Key ka = jbb_key_of(*a);
            uint32_t rank = 0;
            int64_t pred = -1;                                  // the record just below this one
            jbb::Key kp{};
            for (int64_t j = s; j < e; ++j) {
                const OutAln* b = j == i ? nullptr : jb_rec(r, j);
                if (!b) continue;
                const JbCigar cb{(const uint32_t*)b, false};
                const jbb::Key kb = jbb_key_of(*b);
                // a total order: records that compare equal stand in input order
                const bool below = jbb::less(kb, cb, ka, ca) || (j < i && !jbb::less(ka, ca, kb, cb));
                if (!below) continue;
                ++rank;
                const bool above_pred = pred < 0 || jbb::less(kp, JbCigar{(const uint32_t*)&r.slots[pred], false}, kb, cb) ||
                                        (pred < j && !jbb::less(kb, cb, kp, JbCigar{(const uint32_t*)&r.slots[pred], false}));
                if (above_pred) { pred = j; kp = kb; }
            }
            const bool dup = pred >= 0 && jbb::equal(kp, ka);
            if (dup) atomicAdd(&counters[JBB_DUPS], 1ull);
            const uint32_t rl = jbb::read_len(ka.n_cigar, ca);
            o.ref_id = ka.ref_id; o.ref_id2 = ka.ref_id2; o.left = ka.left; o.right = ka.right; o.rank = rank; o.AS = a->AS;
            o.read_len = (uint16_t)(rl > 65535u ? 65535u : rl); o.mismatches = ka.mismatches; o.edit_dist = ka.edit_dist; o.n_cigar = ka.n_cigar;
            bool fused = false;                                 // (the pair grade asks: thj_juncbed_pair_impl.h)
            for (int cc = 0; cc < ka.n_cigar; ++cc) { const uint32_t op = ca(cc) >> 28; fused |= op >= 7u && op <= 10u; }
            const bool contiguous = ka.n_cigar == 1 && (ca(0) >> 28) == 1u;      // one MATCH operation (bwt_map.h:496-499)
            o.flags |= (uint8_t)((dup ? JBB_DUP1 : 0) | (ka.anti ? JBB_ANTI : 0) | (fused ? JBB_FUSED : 0) | (contiguous ? 0 : JBB_SPLICED) | ((a->flags & 4u) ? JBB_ANTI_SPLICE : 0));
        }
        out[i] = o;
    }
}

// exclude_hits_on_filtered_junctions (tophat_reports.cpp:1194-1229) and the AlignStatus score of every record that stays
__global__ __launch_bounds__(256) void thj_k_jbb_score(JbTable t, const JbbRec* rec, int64_t n, const JbOcc* occ, int64_t n_occ, const u64* skey, const uint32_t* acc2,
                                                       const u64* known, int64_t n_known, int max_penalty, int32_t* score) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const JbbRec r = rec[i];
        int32_t sc = JBB_OUT;
        bool ok = !(r.flags & JBB_GONE) && (int64_t)r.jfirst + r.nj <= n_occ;
        for (int k = 0; ok && k < r.nj; ++k) { const uint32_t s = occ[r.jfirst + k].slot; if (s == 0xFFFFFFFFu || !acc2[s]) ok = false; }
        if (ok) {
            const int me = jbb::min_extent(r.read_len);
            sc = r.AS;
            for (int k = 0; k < r.nj; ++k) {
                const u64 key = skey[r.jfirst + k];
                jbb::Seen seen{false, false, 0u, 0u, 0u};
                if (key != JBB_NO_KEY) {
                    seen.annotated = n_known > 0 && jbk::known(known, n_known, key);
                    const uint32_t s = seen.annotated ? 0xFFFFFFFFu : jb_find(t.key, t.mask, key);
                    if (s != 0xFFFFFFFFu && t.cnt1[s] > 0u) { seen.found = true; seen.support = t.cnt1[s]; seen.left_extent = t.le1[s]; seen.right_extent = t.re1[s]; }
                }
                sc = jbb::score_step(sc, seen, max_penalty, me);
            }
        }
        score[i] = sc;
    }
}

// records [s, e) of the read record i belongs to
__device__ __forceinline__ void jbb_read_of(const JbbRec* rec, int64_t n, int64_t i, int64_t& s, int64_t& e) {
    s = i; e = i + 1;
    while (s > 0 && !(rec[s].flags & JBB_FIRST)) --s;
    while (e < n && !(rec[e].flags & JBB_FIRST)) ++e;
}

// read_best_alignments with final_report (tophat_reports.cpp:141-163): the records at the read's maximum, sorted, std::unique
__global__ __launch_bounds__(256) void thj_k_jbb_choose(const JbbRec* rec, int64_t n, const int32_t* score, uint8_t* keep) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t sc = score[i];
        uint8_t kp = 0;
        if (sc != JBB_OUT) {
            int64_t s, e;
            jbb_read_of(rec, n, i, s, e);
            int32_t best = JBB_OUT;
            for (int64_t j = s; j < e; ++j) { const int32_t x = score[j]; best = x > best ? x : best; }
            if (sc == best) {
                const JbbRec me = rec[i];
                int64_t pred = -1; uint32_t prank = 0;
                for (int64_t j = s; j < e; ++j) {
                    if (j == i || score[j] != best) continue;
                    const uint32_t rk = rec[j].rank;
                    if (rk < me.rank && (pred < 0 || rk > prank)) { pred = j; prank = rk; }
                }
                kp = pred >= 0 && jbb::equal(jbb_key_of(rec[pred]), jbb_key_of(me)) ? 0 : 1;
            }
        }
        keep[i] = kp;
    }
}

// per read (the lane of its first record): what is left; over the cap: nothing (--suppress-hits) or listed for the host's generator.
// reports[i] = 1 on the first record of a read of which something is reported, 0 elsewhere.  Whole waves walk together (jb_wave_reserve).
// code (or null): read_best_alignments' return code of every read at its first record (um::read_code: the unmapped-read files and the
// align-summary counters read it after the finish)
__global__ __launch_bounds__(256) void thj_k_jbb_cap(const JbbRec* rec, int64_t n, uint8_t* keep, uint32_t max_multihits, int suppress, uint32_t* reports,
                                                     JbbOver* over, unsigned long long over_cap, unsigned long long* counters, uint8_t* code) {
    const int lane = threadIdx.x & 63;
    const int64_t n_iter = (n + (int64_t)gridDim.x * blockDim.x - 1) / ((int64_t)gridDim.x * blockDim.x);
    for (int64_t it = 0; it < n_iter; ++it) {
        const int64_t i = it * (int64_t)gridDim.x * blockDim.x + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        const bool first = i < n && (rec[i].flags & JBB_FIRST);
        uint32_t left = 0, len = 0; bool lost = false;
        if (first) {
            int64_t e = i + 1;
            while (e < n && !(rec[e].flags & JBB_FIRST)) ++e;
            len = (uint32_t)(e - i);
            for (int64_t j = i; j < e; ++j) { if (keep[j]) ++left; else if (!(rec[j].flags & JBB_GONE)) lost = true; }
        }
        const bool is_over = left > max_multihits;
        if (code && first) code[i] = (uint8_t)um::read_code(left, max_multihits, suppress != 0);
        if (is_over && suppress) { for (int64_t j = i; j < i + len; ++j) keep[j] = 0; left = 0; }
        if (i < n) reports[i] = left ? 1u : 0u;
        const bool list = is_over && !suppress;
        const unsigned long long at = jb_wave_reserve(&counters[JBB_LISTED], list ? 1u : 0u, lane);
        if (list && at < over_cap) over[at] = JbbOver{(u64)i, len, left, 0ull, 0u, 0u};
        const unsigned long long m_first = __ballot(first), m_lost = __ballot(lost), m_over = __ballot(is_over);
        if (lane == 0) {
            if (m_first) atomicAdd(&counters[JBB_READS], (unsigned long long)__popcll(m_first));
            if (m_lost) atomicAdd(&counters[JBB_LOST], (unsigned long long)__popcll(m_lost));
            if (m_over) atomicAdd(&counters[JBB_OVER], (unsigned long long)__popcll(m_over));
        }
    }
}
__global__ __launch_bounds__(256) void thj_k_jbb_before(JbbOver* over, int64_t n_over, const uint32_t* reports_before) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_over; i += (int64_t)gridDim.x * blockDim.x) over[i].before = reports_before[over[i].first];
}
// A wave per listed read: a kept record whose place in rank order among the kept the generator erased (bit clear in mask) gets keep = 2,
// which still counts as a place for the lanes that are counting and as "not kept" for the second pass.
__global__ __launch_bounds__(256) void thj_k_jbb_trim(const JbbRec* rec, uint8_t* keep, const JbbOver* over, int64_t n_over, const uint32_t* mask) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t w = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < n_over; w += waves) {
        const JbbOver o = over[w];
        if (o.pad) continue;                                    // an insert over the cap: thj_k_jbp_apply
        for (int64_t i = (int64_t)o.first + lane; i < (int64_t)(o.first + o.n); i += 64) {
            if (!keep[i]) continue;
            const uint32_t rk = rec[i].rank;
            uint32_t place = 0;
            for (int64_t j = (int64_t)o.first; j < (int64_t)(o.first + o.n); ++j) place += j != i && keep[j] && rec[j].rank < rk;
            if (!((mask[o.word + (place >> 5)] >> (place & 31u)) & 1u)) keep[i] = 2;
        }
    }
}
