// thj_juncbed_fusion_impl.h -- the FusionSet of tophat_reports' consensus pass, reduced beside the JunctionSet (included by
// thj_juncbed_impl.h; what becomes fusions.out).
//
//   update_fusions of both passes                                       tophat_reports.cpp:1156-1180, :2018-2090, :2309-2318
//   fusions_from_alignment, unsupport_fusions, difference                fusions.cpp:44-100, :109-285, :287-343
//   the record walk itself: jbw::fusion, jbw::unsplit_span               thj_jb_walk.h
//
// A read's alignments count only when there are at most fusion_multireads of them, so every add call first counts its records per
// read_idx (a "group"; groups of successive add calls are numbered on).  Add then lists three kinds of occurrence, each with ONE
// reservation per wave:
//   F  a fusion record that passes edit distance and anchors: table slot of its five-field key, left_pos, right_pos, group, and
//      where its junction list starts;  its key enters the pass-1 set (p1 += 1) when its group is small enough
//   U  a record without fusion op and REF_SKIP, read_len() >= 40, that passes edit distance: contig, [left + 20, right() - 20], group
//   J  the junction slots of a record that has REF_SKIPs and is either an F record or belongs to a group larger than
//      fusion_multireads: the junction filter may drop it, which makes its group smaller in pass 2
// Finish, after acc2 is known: J says which records the filter drops (and how many per group); the F occurrences of kept records
// in groups now small enough add count, extents and ONE histogram bin per side (min(pos, 50): left_bases[k] = records with
// left_pos > k, a suffix sum the gather takes); both ends of every pass-1 fusion, sorted by (contig, coordinate), stand for the
// reference's set with its mirror entries, and every U occurrence adds one unsupport per end inside its interval; a workgroup per
// distinct fusion then takes the two 100-base strings from the genome and the five difference() values.
// Every statistic is a sum or a maximum: the order of the records does not matter.
#pragma once

static constexpr uint32_t JBF_NONE = 0xFFFFFFFFu;
static constexpr u64 JBF_NO_JUNC = ~0ull;
static constexpr int JBF_SPIN_LIMIT = 1 << 22;
// counters: distinct keys, overflow flag, F / U / J occurrences written, record flags (1: a record points outside its call's reads or
// the genome), upper bounds of F / U / J counted before the lists grow, ends of the pass-1 set
enum { JBF_DISTINCT = 0, JBF_OVERFLOW, JBF_FOCC, JBF_UOCC, JBF_JOCC, JBF_FLAGS, JBF_FBOUND, JBF_UBOUND, JBF_JBOUND, JBF_ENDS, JBF_N_COUNTERS = 12 };

// the table's layout (JbLayout, thj_juncbed_impl.h)
enum { JBF_K0, JBF_K1, JBF_N64 };
enum { JBF_FID, JBF_P1, JBF_LIST, JBF_N32 };
static constexpr JbLayout JBF_LAYOUT{JBF_N64, JBF_N32, JBF_N_COUNTERS, 1};

struct JbfCfg { int32_t anchor, mismatches, multireads; };
// key: k0 = [ref1 : 32 | left : 32], k1 = [dir - 7 : 2 | ref2 : 30 | right : 32]; fid = the key's number in arrival order; p1 = its pass-1 count
struct JbfTable { u64 *k0, *k1; uint32_t *fid, *p1, *list; u64 mask; unsigned long long* cnt; };
struct JbfOcc { uint32_t slot, left_pos, right_pos, pad; u64 gid, jfirst; };          // 32 bytes
struct JbfUOcc { u64 gid; uint32_t ref, lo, hi, pad; };                                 // 24 bytes
struct JbfJOcc { u64 gid; uint32_t slot; uint8_t nj, idx, dropped, pad; };              // 16 bytes
struct JbfStat { uint32_t count, unsupport, left_ext, right_ext, lh[51], rh[51]; };
static_assert(sizeof(JbfOcc) == 32 && sizeof(JbfUOcc) == 24 && sizeof(JbfJOcc) == 16, "fusion occurrence layouts");
static_assert(sizeof(thj_fusstat) == 660, "thj_fusstat layout");

__device__ __forceinline__ u64 jbf_k0(uint32_t ref1, uint32_t left) { return ((u64)ref1 << 32) | left; }
__device__ __forceinline__ u64 jbf_k1(uint32_t ref2, uint32_t right, uint32_t dir) { return ((u64)(dir - 7u) << 62) | ((u64)ref2 << 32) | right; }

// The key has two words.  Whoever swaps the first word into an empty slot publishes the second at once; a lane that finds the first
// word equal and the second still empty looks at the same slot again.  Everything happens inside the loop body, so the lanes of one
// wave cannot wait for each other; a slot that never gets its second word (it cannot) would end in the overflow flag, not in a hang.
__device__ __forceinline__ uint32_t jbf_insert(const JbfTable& t, u64 a, u64 b) {
    u64 h = jb_mix(a ^ jb_mix(b)) & t.mask;
    uint32_t res = JBF_NONE;
    int probes = 0, spins = 0;
    bool done = false;
    while (!done) {
        u64 cur = __hip_atomic_load(&t.k0[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == ~0ull) {
            const u64 old = atomicCAS((unsigned long long*)&t.k0[h], ~0ull, a);
            if (old == ~0ull) {
                __hip_atomic_store(&t.k1[h], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned long long pos = atomicAdd(&t.cnt[JBF_DISTINCT], 1ull);
                if (pos <= t.mask) t.list[pos] = (uint32_t)h;
                t.fid[h] = (uint32_t)pos;
                res = (uint32_t)h; done = true;
            } else cur = old;
        }
        if (!done) {
            bool next = true;
            if (cur == a) {
                const u64 second = __hip_atomic_load(&t.k1[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (second == b) { res = (uint32_t)h; done = true; next = false; }
                else if (second == ~0ull) { next = false; if (++spins > JBF_SPIN_LIMIT) { atomicExch(&t.cnt[JBF_OVERFLOW], 1ull); done = true; } }
            }
            if (next) {
                h = (h + 1) & t.mask;
                if (++probes >= 4096 || (u64)probes > t.mask) { atomicExch(&t.cnt[JBF_OVERFLOW], 1ull); done = true; }
            }
        }
    }
    return res;
}

// what a record is to the fusion pass
struct JbfRec { bool valid, has, want_f, want_u; unsigned nj; jbw::FusionSite s; uint32_t lo, hi; };
__device__ __forceinline__ JbfRec jbf_classify(const Genome& g, const OutAln& a, bool slot_layout, const JbfCfg& cfg, u64 n_groups, unsigned long long* cnt) {
    JbfRec r{};
    const JbCigar cg{(const uint32_t*)&a, slot_layout};
    const int n = a.n_cigar < SPAN_MAXC ? a.n_cigar : SPAN_MAXC;
    auto ref_ok = [&](uint32_t ref) { return ref >= 1u && ref <= (uint32_t)g.n_contigs; };
    if ((u64)a.read_idx >= n_groups || !ref_ok(a.ref_id)) { atomicOr(&cnt[JBF_FLAGS], 1ull); return r; }
    r.has = jbw::fusion(n, a.left, a.ref_id, cg(SPAN_MAXC - 1), cg, r.s);
    if (r.has && !(ref_ok(r.s.ref1) && ref_ok(r.s.ref2))) { atomicOr(&cnt[JBF_FLAGS], 1ull); return r; }
    r.valid = true;
    r.nj = (unsigned)jb_rec_juncs(a, slot_layout, [](uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) {});
    const bool ed_ok = (int)a.edit_dist <= cfg.mismatches;
    r.want_f = r.has && ed_ok && r.s.inner && r.s.left_pos >= (uint32_t)cfg.anchor && r.s.right_pos >= (uint32_t)cfg.anchor;
    if (!r.has && r.nj == 0 && ed_ok) {
        const jbw::UnsplitSpan u = jbw::unsplit_span(n, a.left, cg);
        r.want_u = u.qualifies;
        r.lo = (uint32_t)a.left + 20u; r.hi = u.right - 20u;
    }
    return r;
}

// group sizes of this add call (grp1 points at the call's first group) and upper bounds for the three lists
__global__ __launch_bounds__(256) void thj_k_jbf_count(Genome g, JbRecs r, JbfCfg cfg, uint32_t* grp1, u64 n_groups, unsigned long long* cnt) {
    __shared__ unsigned int s_f, s_u, s_j;
    if (threadIdx.x == 0) { s_f = 0; s_u = 0; s_j = 0; }
    __syncthreads();
    unsigned int f = 0, u = 0, j = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < r.n_slots + r.n_extra; i += (int64_t)gridDim.x * blockDim.x) {
        const OutAln* a = jb_rec(r, i);
        if (!a) continue;
        const JbfRec x = jbf_classify(g, *a, r.slot_layout, cfg, n_groups, cnt);
        if (!x.valid) continue;
        atomicAdd(&grp1[a->read_idx], 1u);
        f += x.want_f; u += x.want_u; j += x.nj;
    }
    if (f) atomicAdd(&s_f, f);
    if (u) atomicAdd(&s_u, u);
    if (j) atomicAdd(&s_j, j);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_f) atomicAdd(&cnt[JBF_FBOUND], (unsigned long long)s_f);
        if (s_u) atomicAdd(&cnt[JBF_UBOUND], (unsigned long long)s_u);
        if (s_j) atomicAdd(&cnt[JBF_JBOUND], (unsigned long long)s_j);
    }
}

// lists the occurrences of this add call; jt: the junction table, which thj_k_jb_add has filled with the call's junctions already
__global__ __launch_bounds__(256) void thj_k_jbf_add(Genome g, JbRecs r, JbTable jt, JbfTable t, JbfCfg cfg, const uint32_t* grp1, u64 n_groups, u64 grp_base,
                                                     JbfOcc* focc, unsigned long long focc_cap, JbfUOcc* uocc, unsigned long long uocc_cap,
                                                     JbfJOcc* jocc, unsigned long long jocc_cap) {
    const int lane = threadIdx.x & 63;
    const int64_t total = r.n_slots + r.n_extra;
    // whole waves walk together so that the wave-wide reservations see every lane
    const int64_t n_iter = (total + (int64_t)gridDim.x * blockDim.x - 1) / ((int64_t)gridDim.x * blockDim.x);
    for (int64_t it = 0; it < n_iter; ++it) {
        const int64_t i = it * (int64_t)gridDim.x * blockDim.x + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        const OutAln* a = i < total ? jb_rec(r, i) : nullptr;
        JbfRec x{};
        if (a) x = jbf_classify(g, *a, r.slot_layout, cfg, n_groups, t.cnt);
        const uint32_t g1 = x.valid ? grp1[a->read_idx] : 0u;
        const bool small = g1 <= (uint32_t)cfg.multireads;
        const unsigned want_j = x.valid && x.nj && (x.want_f || !small) ? x.nj : 0u;
        const unsigned long long jat = jb_wave_reserve(&t.cnt[JBF_JOCC], want_j, lane);
        const unsigned long long fat = jb_wave_reserve(&t.cnt[JBF_FOCC], x.want_f ? 1u : 0u, lane);
        const unsigned long long uat = jb_wave_reserve(&t.cnt[JBF_UOCC], x.want_u ? 1u : 0u, lane);
        const u64 gid = x.valid ? grp_base + (u64)a->read_idx : 0ull;
        if (want_j) {
            const bool anti = (a->flags & 4u) != 0;             // THJ_HIT_ANTISENSE_SPLICE
            unsigned idx = 0;
            jb_rec_juncs(*a, r.slot_layout, [&](uint32_t ref, uint32_t left, uint32_t right, uint32_t, uint32_t) {
                const uint32_t slot = ref >= 1u && ref <= (uint32_t)g.n_contigs ? jb_find(jt.key, jt.mask, junc_key(g, ref, left, right, anti)) : JBF_NONE;
                if (jat + idx < jocc_cap) jocc[jat + idx] = JbfJOcc{gid, slot, (uint8_t)want_j, (uint8_t)idx, 0, 0};
                ++idx;
            });
        }
        if (x.want_f) {
            const uint32_t slot = jbf_insert(t, jbf_k0(x.s.ref1, x.s.left), jbf_k1(x.s.ref2, x.s.right, x.s.dir));
            if (slot != JBF_NONE && small) atomicAdd(&t.p1[slot], 1u);
            if (fat < focc_cap) focc[fat] = JbfOcc{slot, x.s.left_pos, x.s.right_pos, 0u, gid, want_j ? (u64)jat : JBF_NO_JUNC};
        }
        if (x.want_u && uat < uocc_cap) uocc[uat] = JbfUOcc{gid, a->ref_id, x.lo, x.hi, 0u};
    }
}

// which listed records the junction filter drops (exclude_hits_on_filtered_junctions), and how many of every group
__global__ __launch_bounds__(256) void thj_k_jbf_drop(JbfJOcc* jocc, int64_t n, const uint32_t* acc2, uint32_t* gdrop) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const JbfJOcc o = jocc[i];
        if (o.idx != 0) continue;
        bool ok = true;
        for (int k = 0; k < o.nj && i + k < n; ++k) { const uint32_t s = jocc[i + k].slot; if (s == JBF_NONE || !acc2[s]) ok = false; }
        jocc[i].dropped = ok ? 0 : 1;
        if (!ok) atomicAdd(&gdrop[o.gid], 1u);
    }
}

// pass 2 over the fusion occurrences: a kept record of a group that is now small enough
__global__ __launch_bounds__(256) void thj_k_jbf_second(JbfTable t, const JbfOcc* focc, int64_t n, const JbfJOcc* jocc, int64_t n_jocc, const uint32_t* grp1,
                                                        const uint32_t* gdrop, int multireads, JbfStat* st) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const JbfOcc o = focc[i];
        if (o.slot == JBF_NONE) continue;
        if (o.jfirst != JBF_NO_JUNC && ((int64_t)o.jfirst >= n_jocc || jocc[o.jfirst].dropped)) continue;
        if (grp1[o.gid] - gdrop[o.gid] > (uint32_t)multireads) continue;
        JbfStat* s = &st[t.fid[o.slot]];
        atomicAdd(&s->count, 1u);
        atomicMax(&s->left_ext, o.left_pos);
        atomicMax(&s->right_ext, o.right_pos);
        atomicAdd(&s->lh[o.left_pos < 50u ? o.left_pos : 50u], 1u);
        atomicAdd(&s->rh[o.right_pos < 50u ? o.right_pos : 50u], 1u);
    }
}

__device__ __forceinline__ void jbf_decode(const JbfTable& t, uint32_t slot, jbw::FusionSite& s) {
    const u64 a = t.k0[slot], b = t.k1[slot];
    s.ref1 = (uint32_t)(a >> 32); s.left = (uint32_t)a; s.ref2 = (uint32_t)(b >> 32) & 0x3FFFFFFFu; s.right = (uint32_t)b; s.dir = 7u + (uint32_t)(b >> 62);
}

// both ends of every fusion of the pass-1 set, each with the number of its fusion: the set with its mirror entries (fusions.cpp:210-223).
// A fusion whose two ends are one place is its own mirror and one entry there.
__global__ __launch_bounds__(256) void thj_k_jbf_ends(JbfTable t, int64_t n_f, u64* keys, uint32_t* vals) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_f; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t slot = t.list[i];
        if (t.p1[slot] == 0) continue;
        jbw::FusionSite s; jbf_decode(t, slot, s);
        const bool one = s.ref1 == s.ref2 && s.left == s.right;
        const unsigned long long at = atomicAdd(&t.cnt[JBF_ENDS], one ? 1ull : 2ull);
        keys[at] = jbf_k0(s.ref1, s.left); vals[at] = (uint32_t)i;
        if (!one) { keys[at + 1] = jbf_k0(s.ref2, s.right); vals[at + 1] = (uint32_t)i; }
    }
}

// unsupport_fusions: every end of the pass-1 set on the record's contig inside [left + 20, right() - 20]
__global__ __launch_bounds__(256) void thj_k_jbf_unsupport(const JbfUOcc* uocc, int64_t n, const uint32_t* grp1, const uint32_t* gdrop, int multireads,
                                                           const u64* keys, const uint32_t* vals, int64_t n_ends, JbfStat* st) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const JbfUOcc o = uocc[i];
        if (o.lo > o.hi || grp1[o.gid] - gdrop[o.gid] > (uint32_t)multireads) continue;
        const u64 lo = jbf_k0(o.ref, o.lo), hi = jbf_k0(o.ref, o.hi);
        int64_t a = 0, b = n_ends;                              // lower_bound(lo)
        while (a < b) { const int64_t m = (a + b) >> 1; if (keys[m] < lo) a = m + 1; else b = m; }
        for (int64_t q = a; q < n_ends && keys[q] <= hi; ++q) atomicAdd(&st[vals[q]].unsupport, 1u);
    }
}

// (the reference's window may end one base past the contig, fusions.cpp:234-256: that base is N here)
__device__ __forceinline__ char jbf_base(const Genome& g, uint32_t ref, uint32_t pos, bool complement) {
    if (pos >= (uint32_t)g.contig_len[ref - 1]) return 'N';
    const Planes p = g_fetch(g, ref, (int64_t)pos);
    int code = (p.nm & 1ull) ? 4 : (int)((p.lo & 1ull) | ((p.hi & 1ull) << 1));
    if (complement && code < 4) code = 3 - code;
    return (char)(0x4E54474341ull >> (8 * code));             // "ACGTN", low byte first
}

// difference() of fusions.cpp:44-100 over a[0..len) and b[0..len): two rows of a banded-looking but full table, the minimum over its
// last row and last column.  v0 / v1: `len` int16 each.
__device__ __forceinline__ uint32_t jbf_difference(const char* a, const char* b, int len, int16_t* v0, int16_t* v1) {
    int min_value = 10000;
    int16_t *curr = v0, *prev = v1;
    for (int i = 0; i < len; ++i) { v0[i] = 0; v1[i] = 0; }
    for (int j = 0; j < len; ++j) {
        for (int i = 0; i < len; ++i) {
            int value = 10000;
            const int match = a[i] == b[j] ? 0 : 1;
            if (i == 0) value = j * 2 + match;
            else if (j > 0) value = prev[i] + 2;
            int temp = 10000;
            if (j == 0) temp = i * 2 + match;
            else if (i > 0) temp = curr[i - 1] + 2;
            if (temp < value) value = temp;
            if (i > 0 && j > 0) temp = prev[i - 1] + match;
            if (temp < value) value = temp;
            curr[i] = (int16_t)value;
            if ((i == len - 1 || j == len - 1) && value < min_value) min_value = value;
        }
        int16_t* x = prev; prev = curr; curr = x;
    }
    return (uint32_t)min_value;
}

// a workgroup per distinct fusion, in arrival order (the host drops count == 0 and sorts): the row fusions.out prints
__global__ __launch_bounds__(256) void thj_k_jbf_gather(Genome g, JbfTable t, const JbfStat* st, int64_t n_f, thj_fusstat* out) {
    __shared__ char seq[2][100];
    __shared__ int16_t rows[5][2][100];
    __shared__ int s_strings;
    const int tid = threadIdx.x;
    for (int64_t f = blockIdx.x; f < n_f; f += gridDim.x) {
        jbw::FusionSite s; jbf_decode(t, t.list[f], s);
        const JbfStat* x = &st[f];
        thj_fusstat* o = &out[f];
        if (tid == 0) {
            // fusions.cpp:234-235: both windows inside their contigs
            const u64 len1 = (u64)(uint32_t)g.contig_len[s.ref1 - 1], len2 = (u64)(uint32_t)g.contig_len[s.ref2 - 1];
            s_strings = x->count > 0 && s.left >= 50u && (u64)s.left + 50ull <= len1 && s.right >= 50u && (u64)s.right + 50ull <= len2;
            o->ref_id1 = s.ref1; o->ref_id2 = s.ref2; o->left = s.left; o->right = s.right; o->dir = s.dir;
            o->count = x->count; o->unsupport = x->unsupport; o->left_ext = x->left_ext; o->right_ext = x->right_ext;
            o->n_diffs = s_strings ? 5u : 0u;
        }
        if (tid < 100) {                                       // left_bases[k] = records with left_pos > k
            const uint32_t* h = tid < 50 ? x->lh : x->rh;
            const int k = tid < 50 ? tid : tid - 50;
            uint32_t sum = 0;
            for (int b = k + 1; b <= 50; ++b) sum += h[b];
            (tid < 50 ? o->left_bases : o->right_bases)[k] = sum;
        }
        __syncthreads();
        if (tid < 200) {
            const int side = tid / 100, k = tid % 100;
            char ch = 0;
            if (s_strings) {
                if (side == 0) {                               // :239-245
                    const bool rc = s.dir == 9u || s.dir == 10u;
                    ch = jbf_base(g, s.ref1, rc ? s.left + 49u - (uint32_t)k : s.left - 49u + (uint32_t)k, rc);
                } else {                                       // :247-253
                    const bool rc = s.dir == 8u || s.dir == 10u;
                    ch = jbf_base(g, s.ref2, rc ? s.right + 50u - (uint32_t)k : s.right - 50u + (uint32_t)k, rc);
                }
            }
            seq[side][k] = ch;
            (side == 0 ? o->seq1 : o->seq2)[k] = ch;
        }
        __syncthreads();
        if (tid < 5) {                                         // :258-265: the centred 20, 40, 60, 80 and 100 bases
            const int len = (tid + 1) * 20, pos = (4 - tid) * 10;
            o->diffs[tid] = s_strings ? jbf_difference(seq[0] + pos, seq[1] + pos, len, rows[tid][0], rows[tid][1]) : 0u;
        }
        __syncthreads();
    }
}
