// thj_accepted_pair_impl.h -- accepted_hits.bam for graded inserts, the half that reads the lists thj_juncbed_finish kept (included by
// thj_juncbed_impl.h; the other half, which rewrites the records, is thj_accepted.hip; what they hand each other: thj_accepted_pair.h).
//
// A lane per insert, as in thj_juncbed_pair_impl.h.  An insert that reports pairs (JBP_REPORTS): best_hits = its list walked in sorted order
// without the duplicates (jbp_walk) under the cap's mask; index_vector = lex_hit_sort over the RIGHT records of best_hits, found by counting up
// to 16 entries (ties stand in best_hits order: an insertion sort); for i in that order the right record of pair i, then its left one, each with
// the other as its Mate; CC / CP name the same side's record of the next pair; the primary pair is draw % n (print_sam_for_pair,
// tophat_reports.cpp:1027-1089).  An insert whose sides took the single-end way: the left read's reported records, then the right read's, each
// side counted as thj_k_acc_place counts a read, with its side in the Mate (print_sam_for_single with FRAG_LEFT / FRAG_RIGHT, :2565-2585).
// A list of more than 16 entries is written in hits order and handed to the host for std::sort.
#pragma once
#include "thj_accepted_pair.h"

struct AccpLists {
    const JbbRec* rec; const uint8_t* keep; const int32_t* score; const uint32_t *before, *draw; const JbpIns* ins; const JbpCand* cand;
    const uint32_t *gnk, *gflags, *order, *mword, *mask; const u64* gbig;
};

// best_hits of insert gi: f(k, candidate) for the k-th pair; returns their number
template <class F>
__device__ __forceinline__ uint32_t accp_pairs(const AccpLists& L, int64_t gi, const JbpIns& in, F f) {
    const JbpSrcFinal src{L.rec, L.score};
    const uint32_t mw = L.mword[gi];
    uint32_t k = 0;
    jbp_walk(src, in, L.cand + in.coff, L.gnk[gi], L.gbig[gi] == JBP_SMALL ? nullptr : L.order + L.gbig[gi], [&](uint32_t p, const JbpCand& c) {
        if (mw != 0xFFFFFFFFu && !((L.mask[mw + (p >> 5)] >> (p & 31u)) & 1u)) return;
        f(k, c);
        ++k;
    });
    return k;
}

__global__ __launch_bounds__(256) void thj_k_accp_count(AccpLists L, int64_t g0, int64_t ng, uint32_t* __restrict__ cnt) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < ng; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t gi = g0 + t;
        const JbpIns in = L.ins[gi];
        uint32_t n = 0;
        if (L.gflags[gi] & JBP_REPORTS) n = 2u * accp_pairs(L, gi, in, [](uint32_t, const JbpCand&) {});
        else for (uint32_t k = 0; k < in.nl + in.nr; ++k) n += L.keep[in.first + k] == 1 ? 1u : 0u;
        cnt[t] = n;
    }
}

// the record at ordinal `own` as output record `at` of the call
__device__ __forceinline__ void accp_put(const AccpLists& L, AccPairOut* out, uint32_t at, u64 own, int64_t partner, uint32_t side, uint32_t n, uint32_t place, bool primary, int64_t next,
                                         bool happy) {
    const JbbRec me = L.rec[own];
    AccPairOut o;
    o.rec = (uint32_t)own; o.left = me.left;
    o.slot.n = n; o.slot.place = place; o.slot.ref_id = me.ref_id; o.slot.score = L.score[own]; o.slot.out = at;
    o.slot.flags = (primary ? acc::SLOT_PRIMARY : 0u) | (next >= 0 ? acc::SLOT_HAS_NEXT : 0u);
    o.slot.next_ref = 0; o.slot.next_left = 0;
    if (next >= 0) { const JbbRec nx = L.rec[next]; o.slot.next_ref = nx.ref_id; o.slot.next_left = nx.left; }
    o.mate = acc::Mate();
    o.mate.side = side;
    if (partner >= 0) {
        const JbbRec p = L.rec[partner];
        o.mate.partner = 1u; o.mate.ref_id = p.ref_id; o.mate.left = p.left; o.mate.right = p.right; o.mate.anti = (p.flags & JBB_ANTI) ? 1u : 0u; o.mate.happy = happy ? 1u : 0u;
    }
    out[at] = o;
}

__global__ __launch_bounds__(256) void thj_k_accp_layout(AccpLists L, int64_t g0, int64_t ng, const unsigned long long* __restrict__ base_of, AccPairOut* __restrict__ out,
                                                         AccPairBig* __restrict__ big, uint32_t big_cap, unsigned int* n_big) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < ng; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t gi = g0 + t;
        const JbpIns in = L.ins[gi];
        const uint32_t base = (uint32_t)base_of[t], fl = L.gflags[gi];      // (the caller has looked at the total: below 2^31)
        if (fl & JBP_REPORTS) {
            u64 lo[acc::SORT_BY_COUNTING], ro[acc::SORT_BY_COUNTING];
            const uint32_t n = accp_pairs(L, gi, in, [&](uint32_t k, const JbpCand& c) {
                if (k < acc::SORT_BY_COUNTING) { lo[k] = in.first + c.li; ro[k] = in.first + in.nl + c.rj; }
            });
            if (!n) continue;
            const uint32_t primary = L.draw[L.before[in.first]] % n;
            const bool happy = (fl & JBP_HAPPY) != 0;
            if (n > acc::SORT_BY_COUNTING) {
                accp_pairs(L, gi, in, [&](uint32_t k, const JbpCand& c) {
                    const u64 l = in.first + c.li, r = in.first + in.nl + c.rj;
                    accp_put(L, out, base + 2u * k, r, (int64_t)l, acc::SIDE_RIGHT, n, k, k == primary, -1, happy);
                    accp_put(L, out, base + 2u * k + 1u, l, (int64_t)r, acc::SIDE_LEFT, n, k, k == primary, -1, happy);
                });
                const unsigned int at = atomicAdd(n_big, 1u);
                if (at < big_cap) big[at] = AccPairBig{base, 2u * n, 1u};
                continue;
            }
            for (uint32_t k = 0; k < n; ++k) {
                const JbbRec me = L.rec[ro[k]];
                uint32_t place = 0, nref = 0, nh = 0; int32_t nleft = 0; int nxt = -1;
                for (uint32_t j = 0; j < n; ++j) {
                    if (j == k) continue;
                    const JbbRec r = L.rec[ro[j]];
                    if (acc::lex_before(r.ref_id, r.left, j, me.ref_id, me.left, k)) ++place;
                    else if (nxt < 0 || acc::lex_before(r.ref_id, r.left, j, nref, nleft, nh)) { nxt = (int)j; nref = r.ref_id; nleft = r.left; nh = j; }
                }
                accp_put(L, out, base + 2u * place, ro[k], (int64_t)lo[k], acc::SIDE_RIGHT, n, place, k == primary, nxt < 0 ? -1 : (int64_t)ro[nxt], happy);
                accp_put(L, out, base + 2u * place + 1u, lo[k], (int64_t)ro[k], acc::SIDE_LEFT, n, place, k == primary, nxt < 0 ? -1 : (int64_t)lo[nxt], happy);
            }
            continue;
        }
        // the sides as single reads: the left read's records, then the right read's
        uint32_t sbase = base;
        for (int side = 0; side < 2; ++side) {
            const u64 s = in.first + (side ? in.nl : 0u), e = s + (side ? in.nr : in.nl);
            uint32_t cnt = 0;
            for (u64 j = s; j < e; ++j) cnt += L.keep[j] == 1 ? 1u : 0u;
            if (!cnt) continue;
            const uint32_t primary = L.draw[L.before[s]] % cnt, sd = side ? acc::SIDE_RIGHT : acc::SIDE_LEFT;
            const bool is_big = cnt > acc::SORT_BY_COUNTING;
            for (u64 i = s; i < e; ++i) {
                if (L.keep[i] != 1) continue;
                const JbbRec me = L.rec[i];
                uint32_t hplace = 0, place = 0, nref = 0, nrank = 0; int32_t nleft = 0; int64_t nxt = -1;
                for (u64 j = s; j < e; ++j) {
                    if (j == i || L.keep[j] != 1) continue;
                    const JbbRec r = L.rec[j];
                    hplace += r.rank < me.rank;
                    if (acc::lex_before(r.ref_id, r.left, r.rank, me.ref_id, me.left, me.rank)) ++place;
                    else if (nxt < 0 || acc::lex_before(r.ref_id, r.left, r.rank, nref, nleft, nrank)) { nxt = (int64_t)j; nref = r.ref_id; nleft = r.left; nrank = r.rank; }
                }
                if (is_big) accp_put(L, out, sbase + hplace, i, -1, sd, cnt, hplace, hplace == primary, -1, false);
                else accp_put(L, out, sbase + place, i, -1, sd, cnt, place, hplace == primary, nxt, false);
            }
            if (is_big) {
                const unsigned int at = atomicAdd(n_big, 1u);
                if (at < big_cap) big[at] = AccPairBig{sbase, cnt, 0u};
            }
            sbase += cnt;
        }
    }
}

static int accp_lists(thj_ctx* c, const char* who, int64_t g0, int64_t ng, AccpLists& L) {
    JbState& s = c->jb; JbState::Accepted& A = s.acc; JbState::Pair& P = s.pair;
    if (!A.on || !P.on || !A.chosen || g0 < 0 || ng < 0 || g0 + ng > P.n_ins) { thj_set_error("%s: no insert lists of a finished consensus to read", who); return THJ_ESTATE; }
    L = AccpLists{s.best.rec.p, s.best.keep.p, A.score.p, A.before.p, A.draw.p, P.ins.p, A.p_cand.p, A.p_gnk.p, A.p_gflags.p, A.p_order.p, A.p_mword.p, A.p_mask.p, A.p_gbig.p};
    return THJ_OK;
}

int thj_accp_count(thj_ctx* c, int64_t g0, int64_t ng, uint32_t* d_cnt) {
    AccpLists L;
    if (const int rc = accp_lists(c, "thj_accp_count", g0, ng, L)) return rc;
    if (!ng) return THJ_OK;
    hipLaunchKernelGGL(thj_k_accp_count, jb_grid(ng), dim3(JB_BLOCK), 0, c->stream, L, g0, ng, d_cnt);
    HIPCHK(hipGetLastError());
    return THJ_OK;
}

int thj_accp_layout(thj_ctx* c, int64_t g0, int64_t ng, const unsigned long long* d_base, AccPairOut* d_out, AccPairBig* d_big, uint32_t big_cap, unsigned int* d_nbig) {
    AccpLists L;
    if (const int rc = accp_lists(c, "thj_accp_layout", g0, ng, L)) return rc;
    if (!ng) return THJ_OK;
    hipLaunchKernelGGL(thj_k_accp_layout, jb_grid(ng), dim3(JB_BLOCK), 0, c->stream, L, g0, ng, d_base, d_out, d_big, big_cap, d_nbig);
    HIPCHK(hipGetLastError());
    return THJ_OK;
}
