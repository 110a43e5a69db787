// thj_juncbed_indel_impl.h -- the InsertionSet and the DeletionSet of tophat_reports' second pass, reduced beside the JunctionSet
// (included by thj_juncbed_impl.h; what becomes insertions.bed and deletions.bed).
//
//   update_insertions_and_deletions on the hits exclude_hits_on_filtered_junctions keeps   tophat_reports.cpp:1194-1229, :2286-2313
//   deletions_from_spliced_hit / deletions_from_alignment                                  deletions.cpp:55-72, :83-151
//   insertions_from_spliced_hit / insertions_from_alignment, Insertion::operator<          insertions.cpp:52-70, :109-180, insertions.h:52-67
//
// Pass 1 (thj_k_jb_add<true>) only records: every DEL / dEL / INS / iNS of every record is one 32-byte occurrence -- its key, its
// extents, (record ordinal, op index), the inserted bases, and where the record's junction occurrences start (none: the record
// always counts) -- because which records count is known only after the junction filter.  Pass 2 (finish): an occurrence whose
// record acc2 lets through goes into its table (support += 1, extents = max, atomicMin on (ordinal, op index)); the insertion that
// holds the minimum then writes its letters in a pass of its own: "the first one inserted keeps its letters", std::map::find under
// an operator< that compares lengths only.  The tables are rebuilt by every finish, so a finish can be repeated.
#pragma once

static constexpr int JBI_MAX_INS = 16;                    // inserted bases held per insertion (3 bits each: A C G T N = 0..4)
static constexpr unsigned long long JBI_FLAG_LONG = 1, JBI_FLAG_RANGE = 2, JBI_FLAG_NOSEQ = 4;
static constexpr u64 JBI_NO_JUNC = (1ull << 63) - 1;

// key: deletion = the junction key; insertion = [gpos(left)+1 : 34 | 0 : 22 | length : 8], the stage-1 form with room for 16 bases
// pl = [record ordinal : 40 | op index : 8 | left extent : 16]      br = [bases : 48 | right extent : 16]
// jk = [first junction occurrence of the record, JBI_NO_JUNC: none : 63 | insertion : 1]
struct alignas(16) JbiOcc { u64 key, pl, br, jk; };
static_assert(sizeof(JbiOcc) == 32, "indel occurrence layout");

// where a record's inserted bases come from: ASCII handed in with the records (ins_off[i] .. ins_off[i + 1] = record i's, in cigar
// order), or the read planes of the pass's batch (read_idx, strand, offset in the read); neither: an insertion raises JBI_FLAG_NOSEQ
struct JbiSeq { const int64_t* ins_off; const uint8_t* ins_bases; const u64* planes; const uint16_t* read_len; int W; int64_t n_reads; };

__device__ __forceinline__ u64 jbi_ins_key(const Genome& g, uint32_t ref_id, uint32_t left, uint32_t len) {
    const u64 gpos = (u64)g.contig_blk[ref_id - 1] * 64ull + (u64)(int64_t)(int32_t)left + 1ull;
    return (gpos << 30) | (u64)len;
}
__device__ __forceinline__ uint32_t jbi_ascii_code(uint8_t ch) { return ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u; }

__device__ __forceinline__ int jbi_rec_count(const OutAln& a) {
    const JbCigar cg{(const uint32_t*)&a, false};
    int n = 0;
    for (int c = 0; c < a.n_cigar && c < SPAN_MAXC; ++c) { const uint32_t op = cg(c) >> 28; n += op >= 3 && op <= 6; }
    return n;
}

// the indel occurrences of record `a` (API layout), ordinal `ord`, record i of its add call, written from occ[at] on
__device__ __forceinline__ void jbi_rec_write(const Genome& g, const OutAln& a, int64_t i, u64 ord, u64 jfirst, const JbiSeq& sq, JbiOcc* occ,
                                              unsigned long long at, unsigned long long occ_cap, unsigned long long* flags) {
    const JbCigar cg{(const uint32_t*)&a, false};
    const int n = a.n_cigar < SPAN_MAXC ? a.n_cigar : SPAN_MAXC;
    const uint32_t ref2 = cg(SPAN_MAXC - 1);
    auto clamp16 = [](uint32_t v) { return (u64)(v > 65535u ? 65535u : v); };
    auto ref_ok = [&](uint32_t ref) { return ref >= 1u && ref <= (uint32_t)g.n_contigs; };
    // occurrences of a record lie in op order: deletions and insertions interleaved as the cigar has them
    auto put = [&](int c, u64 key, u64 bases, uint32_t le, uint32_t re, bool ins) {
        int before = 0;
        for (int k = 0; k < c; ++k) { const uint32_t op = cg(k) >> 28; before += op >= 3 && op <= 6; }
        const unsigned long long w = at + (unsigned)before;
        if (w < occ_cap) occ[w] = JbiOcc{key, (ord << 24) | ((u64)(unsigned)c << 16) | clamp16(le), (bases << 16) | clamp16(re), (jfirst << 1) | (ins ? 1ull : 0ull)};
    };
    jbw::dels(n, a.left, a.ref_id, ref2, cg, [&](uint32_t ref, uint32_t left, uint32_t right, uint32_t le, uint32_t re, int c) {
        u64 key = ~0ull;
        if (ref_ok(ref)) key = junc_key(g, ref, left, right, false); else atomicOr(flags, JBI_FLAG_RANGE);
        put(c, key, 0, le, re, false);
    });
    uint32_t taken = 0;                       // inserted bases of this record before the current op
    jbw::inss(n, a.left, a.ref_id, ref2, cg, [&](uint32_t ref, uint32_t left, uint32_t len, uint32_t rpos, uint32_t le, uint32_t re, int c) {
        u64 key = ~0ull, bases = 0;
        if (!ref_ok(ref)) atomicOr(flags, JBI_FLAG_RANGE);
        else if (len > (uint32_t)JBI_MAX_INS) atomicOr(flags, JBI_FLAG_LONG);
        else if (sq.ins_bases) {
            const int64_t b0 = sq.ins_off[i] + taken;
            if (b0 + len > sq.ins_off[i + 1]) atomicOr(flags, JBI_FLAG_RANGE);
            else { key = jbi_ins_key(g, ref, left, len); for (uint32_t k = 0; k < len; ++k) bases |= (u64)jbi_ascii_code(sq.ins_bases[b0 + k]) << (3 * k); }
        } else if (sq.planes) {
            const int rl = (int64_t)a.read_idx < sq.n_reads ? (int)sq.read_len[a.read_idx] : -1;
            if (rl < 0 || rpos + len > (uint32_t)rl || rl > 64 * sq.W) atomicOr(flags, JBI_FLAG_RANGE);
            else {
                SeqView sv; sv.rp = sq.planes + (size_t)a.read_idx * 3 * sq.W; sv.W = sq.W; sv.len = rl; sv.rc = (a.flags & 1u) != 0;      // THJ_HIT_ANTISENSE: SEQ is the read reverse-complemented
                key = jbi_ins_key(g, ref, left, len);
                for (uint32_t k = 0; k < len; ++k) bases |= (u64)(unsigned)seq_code(sv, (int)(rpos + k)) << (3 * k);
            }
        } else atomicOr(flags, JBI_FLAG_NOSEQ);
        taken += len;
        put(c, key, bases, le, re, true);
    });
}

// the layout of one indel table (JbLayout, thj_juncbed_impl.h); the deletion table and the insertion table lie side by side in one
// store and share the counters.  Only the insertion table has priorities and letters.
enum { JBI_KEY, JBI_PRIO, JBI_BASES, JBI_LIST, JBI_N64 };
enum { JBI_CNT, JBI_LE, JBI_RE, JBI_N32 };
enum { JBI_DISTINCT_DEL, JBI_DISTINCT_INS, JBI_OVERFLOW, JBI_N_COUNTERS = 4 };
static constexpr JbLayout JBI_LAYOUT{JBI_N64, JBI_N32, JBI_N_COUNTERS, 2};

struct JbiTable {
    u64 *key, *prio, *bases, *list; u64 mask;
    uint32_t *cnt, *le, *re;
    unsigned long long* distinct;      // distinct keys so far
    unsigned long long* overflow;
};

// second pass: occurrences of the records that exclude_hits_on_filtered_junctions keeps (no REF_SKIP: always; else every junction
// of the record accepted).  n_jocc == 0: no junction was ever seen, acc2 is not read.  keep (best alignments are chosen; null otherwise):
// the records' keep flags by ordinal -- a record that is not kept has no occurrence here.  pcnt, pprio (inserts are graded; null otherwise):
// the reported pairs a record is in -- it counts once per pair -- and, for such a record, the ordinal that stands for its place in the
// reference's order of observation (thj_juncbed_pair_impl.h)
__device__ __forceinline__ uint32_t jbi_times(const JbiOcc& o, const uint8_t* keep, const uint32_t* pcnt, const uint32_t* pprio, u64& prio) {
    prio = o.pl >> 16;
    if (!keep) return 1u;
    const u64 ord = o.pl >> 24;
    const uint32_t pairs = pcnt ? pcnt[ord] : 0u;
    if (pairs) prio = ((u64)pprio[ord] << 8) | (prio & 0xFFu);
    return (keep[ord] == 1 ? 1u : 0u) + pairs;
}
__global__ __launch_bounds__(256) void thj_k_jbi_second(JbiTable del, JbiTable ins, const JbiOcc* occ, int64_t n_occ, const JbOcc* jocc, int64_t n_jocc, const uint32_t* acc2,
                                                        const uint8_t* keep, const uint32_t* pcnt, const uint32_t* pprio) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_occ; i += (int64_t)gridDim.x * blockDim.x) {
        const JbiOcc o = occ[i];
        if (o.key == ~0ull) continue;
        u64 prio;
        const uint32_t times = jbi_times(o, keep, pcnt, pprio, prio);
        if (!times) continue;
        const u64 jf = o.jk >> 1;
        bool ok = true;
        if (jf != JBI_NO_JUNC) {
            if ((int64_t)jf >= n_jocc) continue;
            const int nj = jocc[jf].nj;
            for (int k = 0; k < nj && (int64_t)jf + k < n_jocc; ++k) { const uint32_t s = jocc[jf + k].slot; if (s == 0xFFFFFFFFu || !acc2[s]) ok = false; }
        }
        if (!ok) continue;
        const bool is_ins = (o.jk & 1ull) != 0;
        const JbiTable& t = is_ins ? ins : del;
        const uint32_t slot = jb_insert(t.key, t.mask, t.list, t.distinct, t.overflow, o.key).slot;
        if (slot == 0xFFFFFFFFu) continue;
        atomicAdd(&t.cnt[slot], times);
        atomicMax(&t.le[slot], (uint32_t)(o.pl & 0xFFFFu));
        atomicMax(&t.re[slot], (uint32_t)(o.br & 0xFFFFu));
        if (is_ins) atomicMin((unsigned long long*)&t.prio[slot], (unsigned long long)prio);
    }
}
// the insertion whose (ordinal, op index) won writes its letters; a record the filter dropped never bid, so it cannot match
__global__ __launch_bounds__(256) void thj_k_jbi_letters(JbiTable ins, const JbiOcc* occ, int64_t n_occ, const uint8_t* keep, const uint32_t* pcnt, const uint32_t* pprio) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_occ; i += (int64_t)gridDim.x * blockDim.x) {
        const JbiOcc o = occ[i];
        if (!(o.jk & 1ull) || o.key == ~0ull) continue;
        u64 prio;
        if (pcnt && !jbi_times(o, keep, pcnt, pprio, prio)) continue;      // (places are handed out anew among the records that count: one that does not must not match)
        else if (!pcnt) prio = o.pl >> 16;
        const uint32_t slot = jb_find(ins.key, ins.mask, o.key);
        if (slot != 0xFFFFFFFFu && ins.prio[slot] == prio) ins.bases[slot] = o.br >> 16;
    }
}
struct JbiOut { u64 key, bases; uint32_t support, le, re, pad; };
__global__ __launch_bounds__(256) void thj_k_jbi_gather(JbiTable t, const u64* sorted, int64_t n, JbiOut* out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t s = jb_find(t.key, t.mask, sorted[i]);
        out[i] = JbiOut{sorted[i], t.bases ? t.bases[s] : 0ull, t.cnt[s], t.le[s], t.re[s], 0u};
    }
}
