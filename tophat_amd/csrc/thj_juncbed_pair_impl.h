// thj_juncbed_pair_impl.h -- which alignments of an INSERT count: pair_best_alignments in both of its modes beside the single-end choice
// of thj_juncbed_best_impl.h (included by thj_juncbed_impl.h; the decisions themselves: thj_pair_core.h).
//
// An insert = a left read and a right read with the same number; thj_juncbed_add_pairs lays the records of a call out in the reference's
// visit order (by number; an insert's left records, then its right records) and hands every side to the single-end kernels as a read of
// its own, so ranks, first-pass duplicates and AlignStatus scores are made per record exactly as for single-end input.  A group
// (JbpIns) names an insert's records; one that has one side only is a singleton.
//
// A lane per group, in both passes.  thj_k_jbp_grade generates the candidates left-major, grades them (jbp::grade; the too_far rescue
// looks the gap up in the first-pass junctions of support >= 10, sorted: a binary search to inner1 and a walk to inner2) and writes the
// list pair_best_alignments would hold before its sort.  A list of more than 16 entries goes to the host for libstdc++'s std::sort
// (jbp::sort_order) and comes back as an order; thj_k_jbp_settle then walks every list in sorted order, drops the neighbours that are
// equal under cmp_pair_equal and
//   first pass (at add time, scores = AS, no rescue): counts how many kept pairs every record is in -- thj_k_jb_add adds a record's
//     junctions that many times; no pair kept: every record of both reads once, also the ones over the read filter's limits;
//   second pass (at finish, after thj_k_jbb_score): decides the group's way -- its pairs (a count per record for thj_k_jb_second and
//     thj_k_jbi_second, and the record's place in the reference's order of observation for the insertions' letters: JbpSeen), the
//     single-end second pass for its sides (their scores are handed on to thj_k_jbb_choose / _cap), or nothing -- and lists an insert over
//     --max-multihits for the host's generator beside the single-end reads over the cap; thj_k_jbp_apply takes the generator's answer.
// With the reported alignments collected as well (thj_juncbed_collect_accepted_pairs) the lists, their orders, the flags and the cap's masks stay
// with the context after the finish: thj_accepted_pair_impl.h walks them again to write the inserts' records.
// Most inserts of real input are 1 x 1 and cost one grade.  A wave per insert for the long lists is not built: a lane walks its list alone.
#pragma once
#include "thj_pair_core.h"
#include "thj_unmapped_core.h"

struct JbpCand { int32_t score; uint32_t li, rj, fusion; };     // a kept candidate: the li-th left and the rj-th right record of its group
struct JbpBig { uint32_t g, n; u64 off; };                      // a list for the host: group, entries, where its scores (and its order) lie
enum { JBP_BOTH, JBP_REPORTED, JBP_OVER, JBP_SINGLETONS, JBP_DROPPED, JBP_BIG, JBP_BIGCAND, JBP_N_COUNTERS = 8 };
enum : uint32_t { JBP_BEST_FUSION = 1, JBP_LIVE_L = 2, JBP_LIVE_R = 4, JBP_REPORTS = 8, JBP_HAPPY = 16, JBP_CONC = 32 };       // JBP_HAPPY: happy() of the best grade (accepted hits: flag 0x2); JBP_CONC: its concordant() (the align-summary counters)
static constexpr u64 JBP_SMALL = ~0ull;
static constexpr uint32_t JBP_GIVEN_UP = 0x80000000u;           // in JbbOver::pad of an insert over the cap: its pairs are not reported after all
static constexpr uint32_t JBP_SINGLE_END = 0xFFFFFFFFu;             // first-pass count of a singleton's record: the single-end rule (its JBB_DUP1 flag)
struct JbpResc { const u64* keys; int64_t n; };                 // junction keys of first-pass support >= 10, sorted (Junction::operator< order)

// the records of a pass as the grade reads them: at add time the call's raw records (scores = AS), at finish what was kept of all of them
struct JbpSrcFirst {
    JbRecs r; int64_t base;
    __device__ __forceinline__ bool hit(int64_t o, jbp::Hit& h) const {
        const OutAln* a = jb_rec(r, o - base);
        if (!a) return false;
        const jbb::Key k = jbb_key_of(*a);
        const JbCigar cg{(const uint32_t*)a, false};
        bool fused = false;
        for (int c = 0; c < k.n_cigar; ++c) { const uint32_t op = cg(c) >> 28; fused |= op >= 7u && op <= 10u; }
        h.ref_id = k.ref_id; h.left = k.left; h.right = k.right; h.score = a->AS; h.anti = k.anti; h.fused = fused ? 1 : 0;
        h.spliced = !(k.n_cigar == 1 && (cg(0) >> 28) == 1u); h.anti_splice = (a->flags & 4u) ? 1 : 0;
        return true;
    }
    __device__ __forceinline__ jbb::Key key(int64_t o) const { return jbb_key_of(r.slots[o - base]); }
};
struct JbpSrcFinal {
    const JbbRec* rec; const int32_t* score;
    __device__ __forceinline__ bool hit(int64_t o, jbp::Hit& h) const {
        const int32_t sc = score[o];
        if (sc == JBB_OUT) return false;
        const JbbRec r = rec[o];
        h.ref_id = r.ref_id; h.left = r.left; h.right = r.right; h.score = sc; h.anti = (r.flags & JBB_ANTI) ? 1 : 0; h.fused = (r.flags & JBB_FUSED) ? 1 : 0;
        h.spliced = (r.flags & JBB_SPLICED) ? 1 : 0; h.anti_splice = (r.flags & JBB_ANTI_SPLICE) ? 1 : 0;
        return true;
    }
    __device__ __forceinline__ jbb::Key key(int64_t o) const { return jbb_key_of(rec[o]); }
};

// some junction of support >= 10 on contig `ref` with inner1 <= left, right <= inner2 and the remaining distance inside the window
// dist: the distance the first such junction leaves (jbp::rescued_dist; the keys stand in the set's order)
__device__ __forceinline__ bool jbp_rescue(const Genome& g, const JbpResc& rs, const jbp::Cfg& c, uint32_t ref, int inner1, int inner2, int& dist) {
    if (rs.n <= 0 || ref < 1u || ref > (uint32_t)g.n_contigs || inner1 > inner2) return false;
    const int64_t base = (int64_t)g.contig_blk[ref - 1] * 64;
    const int64_t lo_gp = base + inner1 + 1 < 0 ? 0 : base + inner1 + 1, hi_gp = base + inner2 + 1;
    const u64 lo = (u64)lo_gp << 30;
    int64_t a = 0, b = rs.n;
    while (a < b) { const int64_t m = (a + b) >> 1; if (rs.keys[m] < lo) a = m + 1; else b = m; }
    for (int64_t q = a; q < rs.n && (int64_t)(rs.keys[q] >> 30) <= hi_gp; ++q) {
        const u64 k = rs.keys[q];
        const int64_t jl = (int64_t)(k >> 30) - base - 1, jr = jl + (int64_t)((k >> 1) & ((1ull << 29) - 1));
        if (jbp::rescues((int)jl, (int)jr, 10u, inner1, inner2, c)) { dist = jbp::rescued_dist((int)jl, (int)jr, inner1, inner2); return true; }
    }
    return false;
}

__global__ __launch_bounds__(256) void thj_k_jbp_resc_flags(JbTable t, const u64* sorted, int64_t n, uint8_t* flag) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t s = jb_find(t.key, t.mask, sorted[i]);
        flag[i] = s != 0xFFFFFFFFu && t.cnt1[s] >= 10u ? 1 : 0;
    }
}

// the list of every group before its sort; gflags: whose grade is the best, which sides have records left
template <class Src>
__global__ __launch_bounds__(256) void thj_k_jbp_grade(Src src, Genome g, JbpResc rs, jbp::Cfg cfg, const JbpIns* ins, int64_t n_ins, u64 cand_base, JbpCand* cand,
                                                        uint32_t* gnk, uint32_t* gflags, u64* gbig, JbpBig* big, unsigned long long big_cap, int32_t* bigscore,
                                                        unsigned long long bigscore_cap, unsigned long long* pc) {
    for (int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gi < n_ins; gi += (int64_t)gridDim.x * blockDim.x) {
        const JbpIns in = ins[gi];
        JbpCand* cd = cand + (in.coff - cand_base);
        const uint32_t cap = jbp::side_cap(cfg);
        jbp::Running run{0, 0, 0, 0};
        uint32_t nk = 0, fl = 0, seen_l = 0;
        for (uint32_t i = 0; i < in.nl; ++i) {
            jbp::Hit hl;
            if (!src.hit((int64_t)in.first + i, hl)) continue;
            fl |= JBP_LIVE_L;
            if (!in.nr || ++seen_l > cap) break;
            uint32_t seen_r = 0;
            for (uint32_t j = 0; j < in.nr; ++j) {
                jbp::Hit hr;
                if (!src.hit((int64_t)in.first + in.nl + j, hr)) continue;
                if (++seen_r > cap) break;
                if (!jbp::allowed(hl, hr)) continue;
                const bool fusion = jbp::is_fusion(hl, hr, cfg.fusion_min_dist);
                bool too_far; int inner_after;
                const int sc = jbp::grade_dist(hl, hr, cfg, fusion, [&](uint32_t ref, int inner1, int inner2, int& d) { return jbp_rescue(g, rs, cfg, ref, inner1, inner2, d); }, too_far, inner_after);
                const int act = jbp::step(run, sc, fusion, cfg, jbp::happy(hl, hr, too_far), jbp::concordant(hl, hr, inner_after, cfg));
                if (act == jbp::STEP_CLEAR_ENTER) nk = 0;
                if (act != jbp::STEP_SKIP) cd[nk++] = JbpCand{sc, i, j, fusion ? 1u : 0u};
            }
        }
        for (uint32_t j = 0; j < in.nr; ++j) { jbp::Hit hr; if (src.hit((int64_t)in.first + in.nl + j, hr)) { fl |= JBP_LIVE_R; break; } }
        if (run.best_fusion) fl |= JBP_BEST_FUSION;
        if (run.best_happy) fl |= JBP_HAPPY;
        if (run.best_conc) fl |= JBP_CONC;
        u64 off = JBP_SMALL;
        if (nk > jbp::SORT_SMALL) {
            const unsigned long long at = atomicAdd(&pc[JBP_BIG], 1ull), o = atomicAdd(&pc[JBP_BIGCAND], (unsigned long long)nk);
            if (at < big_cap && o + nk <= bigscore_cap) {
                big[at] = JbpBig{(uint32_t)gi, nk, (u64)o};
                for (uint32_t k = 0; k < nk; ++k) bigscore[o + k] = cd[k].score;
                off = (u64)o;
            } else nk = 0;                                      // (cannot happen: both capacities are the host's exact bounds)
        }
        gnk[gi] = nk; gflags[gi] = fl; gbig[gi] = off;
    }
}

// a group's list in sorted order without the neighbours equal under cmp_pair_equal: f(place among the survivors, entry); returns their number
template <class Src, class F>
__device__ __forceinline__ uint32_t jbp_walk(const Src& src, const JbpIns& in, const JbpCand* cd, uint32_t nk, const uint32_t* order, F f) {
    uint8_t ord[jbp::SORT_SMALL];
    if (!order) for (uint32_t a = 0; a < nk; ++a) ord[jbp::place16(nk, a, [&](uint32_t k) { return cd[k].score; })] = (uint8_t)a;
    uint32_t n_left = 0;
    jbb::Key pl{}, pr{};
    for (uint32_t p = 0; p < nk; ++p) {
        const uint32_t a = order ? order[p] : ord[p];
        if (a >= nk) continue;
        const JbpCand c = cd[a];
        const jbb::Key kl = src.key((int64_t)in.first + c.li), kr = src.key((int64_t)in.first + in.nl + c.rj);
        if (n_left && jbb::equal(pl, kl) && jbb::equal(pr, kr)) continue;
        pl = kl; pr = kr;
        f(n_left, c);
        ++n_left;
    }
    return n_left;
}
__device__ __forceinline__ void jbp_bump(uint32_t* x) { ++*x; }
// A reported pair's two records are counted, and a record seen for the first time takes the next place of its side: update_junctions and
// update_insertions_and_deletions see an insert's left records in pair-list order, then its right records in pair-list order
// (tophat_reports.cpp:2502-2519), and of two equal insertions the first one seen keeps its letters.  Places are ordinals inside the insert's own
// range -- left from in.first, right from in.first + in.nl -- so they order against every other insert's as the visit does.
struct JbpSeen {
    uint32_t* pcnt; uint32_t* pprio; uint32_t next_l, next_r;
    __device__ __forceinline__ void pair(const JbpIns& in, const JbpCand& c) {
        const u64 l = in.first + c.li, r = in.first + in.nl + c.rj;
        if (!pcnt[l]++) pprio[l] = next_l++;
        if (!pcnt[r]++) pprio[r] = next_r++;
    }
};

// first pass: mult[record of the call] = the kept pairs it is in (host: 0 for an insert's records, JBP_SINGLE_END for a singleton's)
__global__ __launch_bounds__(256) void thj_k_jbp_settle_first(JbpSrcFirst src, const JbpIns* ins, int64_t n_ins, u64 cand_base, const JbpCand* cand, const uint32_t* gnk,
                                                               const u64* gbig, const uint32_t* order, uint32_t* mult, uint8_t* unflt) {
    for (int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gi < n_ins; gi += (int64_t)gridDim.x * blockDim.x) {
        const JbpIns in = ins[gi];
        if (!in.nl || !in.nr) continue;
        const int64_t at = (int64_t)in.first - src.base;
        const uint32_t n_left = jbp_walk(src, in, cand + (in.coff - cand_base), gnk[gi], gbig[gi] == JBP_SMALL ? nullptr : order + gbig[gi],
                                         [&](uint32_t, const JbpCand& c) { jbp_bump(&mult[at + c.li]); jbp_bump(&mult[at + in.nl + c.rj]); });
        // no pair: the hit groups as they came (tophat_reports.cpp:2075-2079)
        if (!n_left) for (uint32_t k = 0; k < in.nl + in.nr; ++k) { mult[at + k] = 1; unflt[at + k] = 1; }
    }
}

// second pass: score1 = the scores of the records that take the single-end way (JBB_OUT elsewhere), pcnt = the reported pairs a record is
// in, the inserts over the cap appended to the single-end list (n = ties, pad = the entries above them + 1, JBP_GIVEN_UP on top when the insert
// takes the single-end way after all; pad 0 marks a single-end read)
__global__ __launch_bounds__(256) void thj_k_jbp_settle(JbpSrcFinal src, jbp::Cfg cfg, const JbpIns* ins, int64_t n_ins, const JbpCand* cand, const uint32_t* gnk, uint32_t* gflags,
                                                         const u64* gbig, const uint32_t* order, int32_t* score1, uint32_t* pcnt, uint32_t* pprio, JbbOver* over, unsigned long long over_cap,
                                                         unsigned long long* listed, unsigned long long* pc, uint32_t* iword) {
    const int lane = threadIdx.x & 63;
    const int64_t n_iter = (n_ins + (int64_t)gridDim.x * blockDim.x - 1) / ((int64_t)gridDim.x * blockDim.x);
    for (int64_t it = 0; it < n_iter; ++it) {
        const int64_t gi = it * (int64_t)gridDim.x * blockDim.x + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        bool both = false, reported = false, is_over = false, single = false;
        uint32_t dropped = 0;
        if (gi < n_ins) {
            const JbpIns in = ins[gi];
            const uint32_t fl = gflags[gi], nk = gnk[gi];
            const JbpCand* cd = cand + in.coff;
            const uint32_t* ord = gbig[gi] == JBP_SMALL ? nullptr : order + gbig[gi];
            const bool live_l = fl & JBP_LIVE_L, live_r = fl & JBP_LIVE_R;
            both = in.nl && in.nr; single = !both;
            int way = 0;                                        // 0 nothing, 1 the sides as single reads, 2 its pairs
            uint32_t n_left = 0;
            if (!both || !live_l || !live_r) {
                way = cfg.report_mixed ? 1 : 0;
                if (!cfg.report_mixed) dropped = (live_l ? 1u : 0u) + (live_r ? 1u : 0u);
            } else {
                int32_t tie = 0;
                n_left = jbp_walk(src, in, cd, nk, ord, [&](uint32_t p, const JbpCand& c) { if (p + 1 == (uint32_t)cfg.max_multihits) tie = c.score; });
                is_over = n_left > (uint32_t)cfg.max_multihits;
                uint32_t left = is_over && cfg.suppress ? 0u : n_left;
                if (cfg.report_mixed && (!left || ((fl & JBP_BEST_FUSION) && !cfg.report_discordant))) way = 1;
                else way = left ? 2 : 0;
                if (is_over && !cfg.suppress) {
                    // the cap's draws are made inside pair_best_alignments, also when the pairs are then given up for the single-end way
                    uint32_t better = 0, ties = 0;
                    jbp_walk(src, in, cd, nk, ord, [&](uint32_t, const JbpCand& c) { better += c.score > tie; ties += c.score == tie; });
                    const unsigned long long at = atomicAdd(listed, 1ull);
                    if (at < over_cap) over[at] = JbbOver{in.first, ties, n_left, 0ull, 0u, (better + 1u) | (way == 2 ? 0u : JBP_GIVEN_UP)};
                } else if (way == 2) {
                    JbpSeen seen{pcnt, pprio, (uint32_t)in.first, (uint32_t)(in.first + in.nl)};
                    jbp_walk(src, in, cd, nk, ord, [&](uint32_t, const JbpCand& c) { seen.pair(in, c); });
                }
            }
            reported = way == 2;
            gflags[gi] = reported ? fl | JBP_REPORTS : fl;
            if (iword) {                                        // the unmapped-read files and the align-summary counters: the way the worker loop takes (um::insert_word)
                bool gone_l = false, gone_r = false;
                for (uint32_t k = 0; k < in.nl; ++k) gone_l |= (src.rec[in.first + k].flags & JBB_GONE) != 0;
                for (uint32_t k = 0; k < in.nr; ++k) gone_r |= (src.rec[in.first + in.nl + k].flags & JBB_GONE) != 0;
                iword[gi] = um::insert_word(in.nl != 0u, in.nr != 0u, live_l, live_r, gone_l, gone_r, n_left, (fl & JBP_BEST_FUSION) != 0u, (fl & JBP_CONC) != 0u,
                                            (uint32_t)cfg.max_multihits, cfg.suppress != 0, cfg.report_mixed != 0, cfg.report_discordant != 0);
            }
            for (uint32_t k = 0; k < in.nl + in.nr; ++k) score1[in.first + k] = way == 1 ? src.score[in.first + k] : JBB_OUT;
        }
        const unsigned long long m_both = __ballot(both), m_rep = __ballot(reported), m_over = __ballot(is_over), m_single = __ballot(single && gi < n_ins);
        unsigned int d = dropped;
        for (int s = 32; s; s >>= 1) d += __shfl_xor(d, s);
        if (lane == 0) {
            if (m_both) atomicAdd(&pc[JBP_BOTH], (unsigned long long)__popcll(m_both));
            if (m_rep) atomicAdd(&pc[JBP_REPORTED], (unsigned long long)__popcll(m_rep));
            if (m_over) atomicAdd(&pc[JBP_OVER], (unsigned long long)__popcll(m_over));
            if (m_single) atomicAdd(&pc[JBP_SINGLETONS], (unsigned long long)__popcll(m_single));
            if (d) atomicAdd(&pc[JBP_DROPPED], (unsigned long long)d);
        }
    }
}

// after thj_k_jbb_cap: an insert of which a pair is reported draws once (print_sam_for_pair), at its first record
__global__ __launch_bounds__(256) void thj_k_jbp_reports(const JbpIns* ins, int64_t n_ins, const uint32_t* gflags, uint32_t* reports) {
    for (int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gi < n_ins; gi += (int64_t)gridDim.x * blockDim.x)
        if (gflags[gi] & JBP_REPORTS) reports[ins[gi].first] = 1u;
}

// the generator's answer for the inserts over the cap: bit p of the mask = the survivor at place p stays; mword (or null): per insert, where its bits begin
__global__ __launch_bounds__(256) void thj_k_jbp_apply(JbpSrcFinal src, const JbpIns* ins, int64_t n_ins, const JbpCand* cand, const uint32_t* gnk, const u64* gbig,
                                                        const uint32_t* order, const JbbOver* over, int64_t n_over, const uint32_t* mask, uint32_t* pcnt, uint32_t* pprio, uint32_t* mword) {
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_over; w += (int64_t)gridDim.x * blockDim.x) {
        const JbbOver o = over[w];
        if (!o.pad || (o.pad & JBP_GIVEN_UP)) continue;
        int64_t a = 0, b = n_ins;                               // the group that starts at o.first (groups lie in record order)
        while (a < b) { const int64_t m = (a + b) >> 1; if (ins[m].first < o.first) a = m + 1; else b = m; }
        if (a >= n_ins || ins[a].first != o.first) continue;
        const JbpIns in = ins[a];
        if (mword) mword[a] = o.word;                           // (accepted hits: the report walks the list under the same bits)
        JbpSeen seen{pcnt, pprio, (uint32_t)in.first, (uint32_t)(in.first + in.nl)};
        jbp_walk(src, in, cand + in.coff, gnk[a], gbig[a] == JBP_SMALL ? nullptr : order + gbig[a], [&](uint32_t p, const JbpCand& c) {
            if ((mask[o.word + (p >> 5)] >> (p & 31u)) & 1u) seen.pair(in, c);
        });
    }
}
