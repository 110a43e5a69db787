// thj_accepted.hip -- accepted_hits.bam's records on the device (thj_juncbed_report_bam): after thj_juncbed_finish has chosen which
// alignments of every read are reported, the inputs are replayed piece by piece and every reported record is rewritten the way
// print_sam_for_single / rewrite_sam_record write it (tophat_reports.cpp:985-1025, :656-781, :580-654).  The decisions: thj_accepted_core.h.
//
// Per piece (inflated and parsed again by thj_ingest_reported; the choice -- JbbRec, keep flags, scores, draws -- stayed on the device):
//   thj_k_acc_kept    a lane per record: reported or not; the read runs must be the runs of the add call (LOUD_ORDER otherwise)
//   thj_k_acc_place   a lane per reported record: it counts over its read's run as thj_k_jbb_choose does -- n, its place in `hits` (rank
//                     order), its place in index_vector (lex_hit_sort by counting: ties stand in hits order, which is what std::sort gives
//                     up to 16 entries), the record behind it, whether it is the primary (draw % n).  Reads of more than 16 reported
//                     alignments are listed: the host runs std::sort itself on them (acc::sort_places) and writes their places.
//   thj_k_acc_plan    a lane per reported record: emit() with the counting sink -> its size at its output place, the loud flags
//   (scan)            sizes -> offsets; a read's records lie in index_vector order, reads in input order
//   thj_k_acc_write   a WAVE per reported record: emit() again, every lane running the same walk (its branches are uniform); spans that
//                     come out as they went in -- QNAME, SEQ, QUAL, runs of unchanged tags -- move with all 64 lanes, the patched header
//                     words and the re-encoded or appended tags are written by lane 0.
// Graded inserts (thj_juncbed_report_pairs_bam): the records come from the host as it read them, a side each; thj_accepted_pair_impl.h lays
// every insert's output records out (source record, Slot, Mate) from the lists the finish kept, and the same three steps follow per OUTPUT
// record -- thj_k_accp_plan, the scan, thj_k_accp_write with the same sink.
// Records start at any byte on both sides.  The stores stay wide by aligning the DESTINATION: up to three bytes bring it to a 4-byte
// boundary, then every lane stores one aligned dword that it puts together from the two aligned source dwords its four bytes lie in
// (a funnel shift by the sides' misalignment), then up to three bytes finish; 64 lanes x 4 bytes is a full 256-byte request per
// instruction.  Wider stores would help spans of kilobytes; a record's spans are tens to a few hundred bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/thj.h"
#include "thj_ctx.h"
#include "thj_scan.h"
#include "thj_jbb_rec.h"
#include "thj_accepted_core.h"
#include "thj_accepted_pair.h"
#include "thj_wave_sink.h"

namespace {

enum { ACC_LOUD, ACC_BIG, ACC_N_COUNTERS = 4 };
struct AccBig { uint32_t s, e; };                                // a read of more than 16 reported alignments: records [s, e) of the piece

__device__ __forceinline__ const uint8_t* acc_rec_at(const uint8_t* infl, uint32_t loc) { return infl + ((size_t)(loc >> 16) << 16) + (loc & 0xFFFFu); }

__global__ __launch_bounds__(256) void thj_k_acc_kept(const JbbRec* __restrict__ rec, const uint8_t* __restrict__ keep, const thj_aln* __restrict__ aln, int64_t n,
                                                      uint32_t* __restrict__ kept, unsigned int* counters) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        kept[i] = keep[i] == 1 ? 1u : 0u;
        const bool first_then = (rec[i].flags & JBB_FIRST) != 0, first_now = i == 0 || aln[i].read_idx != aln[i - 1].read_idx;
        if (first_then != first_now) atomicOr(&counters[ACC_LOUD], (unsigned int)acc::LOUD_ORDER);
    }
}

// rec / score: this piece's records of the consensus (B.rec + ordinal base ...); before: the reporting reads before every record of the
// consensus, at the same base; draw[k] = the generator's output for the k-th reporting read
__global__ __launch_bounds__(256) void thj_k_acc_place(const JbbRec* __restrict__ rec, const int32_t* __restrict__ score, const uint32_t* __restrict__ before,
                                                       const uint32_t* __restrict__ draw, const uint32_t* __restrict__ kept, const uint32_t* __restrict__ kb, int64_t n,
                                                       acc::Slot* __restrict__ slot, AccBig* __restrict__ big, unsigned int big_cap, unsigned int* counters) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (!kept[i]) continue;
        int64_t s = i, e = i + 1;
        while (s > 0 && !(rec[s].flags & JBB_FIRST)) --s;
        while (e < n && !(rec[e].flags & JBB_FIRST)) ++e;
        const JbbRec me = rec[i];
        uint32_t cnt = 0, hplace = 0, place = 0;
        int64_t nxt = -1; uint32_t nref = 0, nrank = 0; int32_t nleft = 0;
        for (int64_t j = s; j < e; ++j) {
            if (!kept[j]) continue;
            ++cnt;
            if (j == i) continue;
            const uint32_t r = rec[j].ref_id, rk = rec[j].rank; const int32_t l = rec[j].left;
            hplace += rk < me.rank;
            if (acc::lex_before(r, l, rk, me.ref_id, me.left, me.rank)) ++place;
            else if (nxt < 0 || acc::lex_before(r, l, rk, nref, nleft, nrank)) { nxt = j; nref = r; nleft = l; nrank = rk; }
        }
        acc::Slot o;
        o.n = cnt; o.place = place; o.ref_id = me.ref_id; o.next_ref = nref; o.next_left = nleft; o.score = score[i];
        o.flags = (hplace == draw[before[s]] % cnt ? acc::SLOT_PRIMARY : 0u) | (nxt >= 0 ? acc::SLOT_HAS_NEXT : 0u);
        o.out = kb[s] + place;
        slot[i] = o;
        if (cnt > acc::SORT_BY_COUNTING && kb[i] == kb[s]) {     // the read's first reported record lists it
            const unsigned int at = atomicAdd(&counters[ACC_BIG], 1u);
            if (at < big_cap) big[at] = AccBig{(uint32_t)s, (uint32_t)e};
        }
    }
}

__global__ __launch_bounds__(256) void thj_k_acc_plan(const uint8_t* __restrict__ infl, const uint32_t* __restrict__ loc, const uint32_t* __restrict__ kept,
                                                      const acc::Slot* __restrict__ slot, int64_t n, acc::Cfg cfg, uint32_t* __restrict__ size_out, unsigned int* counters,
                                                      unsigned long long* in_bytes) {
    unsigned long long mine = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (!kept[i]) continue;
        const uint8_t* p = acc_rec_at(infl, loc[i]);
        const uint32_t bs = acc::rd32(p);
        acc::NullSink sink;
        uint32_t loud = 0;
        const acc::Slot s = slot[i];
        const uint32_t size = acc::emit(p + 4, bs, cfg, s, sink, loud);
        size_out[s.out] = size;
        if (loud) atomicOr(&counters[ACC_LOUD], loud);
        mine += bs + 4u;
    }
    if (mine) atomicAdd(in_bytes, mine);
}

__global__ __launch_bounds__(256) void thj_k_acc_write(const uint8_t* __restrict__ infl, const uint32_t* __restrict__ loc, const uint32_t* __restrict__ kept,
                                                       const acc::Slot* __restrict__ slot, int64_t n, acc::Cfg cfg, const unsigned long long* __restrict__ off, uint8_t* out) {
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t i = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < n; i += waves) {
        if (!kept[i]) continue;
        const uint8_t* p = acc_rec_at(infl, loc[i]);
        const uint32_t bs = acc::rd32(p);
        const acc::Slot s = slot[i];
        WaveSink sink{out + off[s.out], lane};
        uint32_t loud = 0;
        (void)acc::emit(p + 4, bs, cfg, s, sink, loud);
    }
}

// scratch of one call from the context's block cache: the stream idle first, then back to the cache, on every way out
struct AccScratch {
    thj_ctx* c; void* p = nullptr;
    explicit AccScratch(thj_ctx* c_) : c(c_) {}  AccScratch(const AccScratch&) = delete;
    ~AccScratch() { if (!p) return; (void)hipStreamSynchronize(c->stream); thj_dev_release(c, p); }
};
template <class T>
int acc_grow(DevBuf<T>& b, size_t need) {
    if ((int64_t)need <= b.cap) return THJ_OK;
    b.release();
    HIPCHK(hipMalloc((void**)&b.p, need * sizeof(T)));
    b.cap = (int64_t)need;
    return THJ_OK;
}
dim3 acc_grid(int64_t n) { const int64_t b = (n + 255) / 256; return dim3((unsigned)(b > 4096 ? 4096 : b < 1 ? 1 : b)); }

// ---- graded inserts (thj_juncbed_report_pairs_bam): the output records are laid out by thj_accepted_pair_impl.h; raw = the call's input records
// as the host gave them (left side, then right side), src_off[record of the call, in the consensus' order] = where its block_size field lies
__global__ __launch_bounds__(256) void thj_k_accp_plan(const uint8_t* __restrict__ raw, const unsigned long long* __restrict__ src_off, uint32_t first_rec,
                                                       const AccPairOut* __restrict__ outs, int64_t n_out, acc::Cfg cfg, uint32_t* __restrict__ size_out, unsigned int* counters) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += (int64_t)gridDim.x * blockDim.x) {
        const AccPairOut o = outs[i];
        const uint8_t* p = raw + src_off[o.rec - first_rec];
        acc::NullSink sink;
        uint32_t loud = 0;
        size_out[i] = acc::emit(p + 4, acc::rd32(p), cfg, o.slot, sink, loud, o.mate);
        if (loud) atomicOr(&counters[ACC_LOUD], loud);
    }
}
__global__ __launch_bounds__(256) void thj_k_accp_write(const uint8_t* __restrict__ raw, const unsigned long long* __restrict__ src_off, uint32_t first_rec,
                                                        const AccPairOut* __restrict__ outs, int64_t n_out, acc::Cfg cfg, const unsigned long long* __restrict__ off, uint8_t* out) {
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t i = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < n_out; i += waves) {
        const AccPairOut o = outs[i];
        const uint8_t* p = raw + src_off[o.rec - first_rec];
        WaveSink sink{out + off[i], lane};
        uint32_t loud = 0;
        (void)acc::emit(p + 4, acc::rd32(p), cfg, o.slot, sink, loud, o.mate);
    }
}

}  // namespace

extern "C" int thj_juncbed_report_bam(thj_ctx* c, const thj_bam_piece* piece, int32_t max_report_intron, int32_t more_follows, int64_t* n_records,
                                      uint32_t* resume_member, uint32_t* resume_skip, uint32_t* rec_size, int64_t rec_cap, int64_t* total_bytes) {
    if (!c || !piece || piece->comp_bytes < 0 || (piece->comp_bytes > 0 && !piece->comp) || piece->n_tid < 0 || (piece->n_tid > 0 && !piece->tid2ref) || !n_records ||
        !resume_member || !resume_skip || rec_cap < 0 || (rec_cap > 0 && !rec_size) || !total_bytes) { thj_set_error("thj_juncbed_report_bam: bad argument"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    JbState& S = c->jb; JbState::Accepted& A = S.acc; JbState::Best& B = S.best;
    *n_records = 0; *resume_member = 0; *resume_skip = 0;
    if (!A.on || !B.on) { thj_set_error("thj_juncbed_report_bam: the pass was not armed (thj_juncbed_collect_accepted between the reset and the first add)"); return THJ_ESTATE; }
    if (!A.chosen) { thj_set_error("thj_juncbed_report_bam: no choice has been made yet (thj_juncbed_finish first)"); return THJ_ESTATE; }
    int64_t added = 0;
    for (int64_t x : A.calls) added += x;
    if (added != S.records) { thj_set_error("thj_juncbed_report_bam: records were added by other calls than thj_juncbed_add_bam: only pieces can be replayed"); return THJ_ESTATE; }
    if (A.replayed >= A.calls.size()) { thj_set_error("thj_juncbed_report_bam: every add call of this consensus has been replayed already (%zu)", A.calls.size()); return THJ_ESTATE; }
    if (A.replayed == 0) c->bam_bytes = 0;                       // the first piece opens the stream
    *total_bytes = c->bam_bytes;
    if (!c->d_contig_names || c->n_contig_names != c->n_contigs) { thj_set_error("thj_juncbed_report_bam: the context holds no names for the genome's %d contigs (thj_bam_contig_names_upload)", (int)c->n_contigs); return THJ_ESTATE; }
    thj_reported_recs r;
    if (const int rc = thj_ingest_reported(c, piece, max_report_intron, 0, 0, 1, more_follows, &r)) return rc;
    *resume_member = r.resume_member; *resume_skip = r.resume_skip;
    if (r.n != A.calls[A.replayed]) {
        thj_set_error("thj_juncbed_report_bam: %s (piece %zu gave %lld records, its add call %lld)", acc::loud_text(acc::LOUD_ORDER), A.replayed, (long long)r.n, (long long)A.calls[A.replayed]);
        return THJ_EINVAL;
    }
    const int64_t n = r.n, ord0 = A.replayed_records;
    if (n == 0) { ++A.replayed; return THJ_OK; }
    // scratch: [kept | kb | size_out] (n + 1 each), offsets (n + 1), slots (n), the list of large reads, the counters, the input bytes
    const size_t n1 = (size_t)n + 1, big_cap = (size_t)n / (acc::SORT_BY_COUNTING + 1) + 1;
    const size_t b_u32 = (n1 * 4 + 15) & ~(size_t)15, b_off = n1 * 8, b_slot = (size_t)n * sizeof(acc::Slot), b_big = (big_cap * sizeof(AccBig) + 15) & ~(size_t)15;
    AccScratch scratch(c);
    if (const int rc = thj_dev_alloc(c, &scratch.p, 3 * b_u32 + b_off + b_slot + b_big + 64)) return rc;
    char* d = (char*)scratch.p;
    unsigned long long* off = (unsigned long long*)d;
    acc::Slot* slot = (acc::Slot*)(d + b_off);
    uint32_t *kept = (uint32_t*)(d + b_off + b_slot), *kb = (uint32_t*)((char*)kept + b_u32), *size_out = (uint32_t*)((char*)kb + b_u32);
    AccBig* big = (AccBig*)((char*)size_out + b_u32);
    unsigned int* counters = (unsigned int*)((char*)big + b_big);
    unsigned long long* in_bytes = (unsigned long long*)(counters + ACC_N_COUNTERS);
    HIPCHK(hipMemsetAsync(counters, 0, ACC_N_COUNTERS * 4 + 8, c->stream));
    HIPCHK(hipMemsetAsync(kept + n, 0, 4, c->stream));
    HIPCHK(hipMemsetAsync(size_out, 0, n1 * 4, c->stream));
    const JbbRec* rec = B.rec.p + ord0;
    hipLaunchKernelGGL(thj_k_acc_kept, acc_grid(n), dim3(256), 0, c->stream, rec, (const uint8_t*)B.keep.p + ord0, (const thj_aln*)r.recs, n, kept, counters);
    if (const int e = ensure_sort_tmp(c, std::max(thj_scan::scratch_bytes((int64_t)n1, 8), (size_t)1 << 20))) return e;
    thj_scan::exclusive_sum<uint32_t, uint32_t>(c->stream, kept, kb, (int64_t)n1, c->d_sort_tmp);
    hipLaunchKernelGGL(thj_k_acc_place, acc_grid(n), dim3(256), 0, c->stream, rec, (const int32_t*)A.score.p + ord0, (const uint32_t*)A.before.p + ord0,
                       (const uint32_t*)A.draw.p, (const uint32_t*)kept, (const uint32_t*)kb, n, slot, big, (unsigned int)big_cap, counters);
    HIPCHK(hipGetLastError());
    unsigned int h_cnt[ACC_N_COUNTERS];
    uint32_t n_out = 0;
    HIPCHK(hipMemcpyAsync(h_cnt, counters, sizeof h_cnt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&n_out, kb + n, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (h_cnt[ACC_LOUD] & acc::LOUD_ORDER) { thj_set_error("thj_juncbed_report_bam: %s", acc::loud_text(acc::LOUD_ORDER)); return THJ_EINVAL; }
    if ((int64_t)n_out > rec_cap) { thj_set_error("thj_juncbed_report_bam: room for %lld record sizes, the piece reports %u records", (long long)rec_cap, n_out); return THJ_EINVAL; }
    if (h_cnt[ACC_BIG]) {
        // reads of more than 16 reported alignments: std::sort itself, on the sequence the reference sorts (hits in rank order) with its comparator
        const size_t nb = h_cnt[ACC_BIG];
        if (nb > big_cap) { thj_set_error("thj_juncbed_report_bam: more large reads than records allow"); return THJ_EINVAL; }
        std::vector<AccBig> list(nb);
        HIPCHK(hipMemcpy(list.data(), big, nb * sizeof(AccBig), hipMemcpyDeviceToHost));
        uint32_t lo = 0xFFFFFFFFu, hi = 0;
        for (const AccBig& g : list) { lo = std::min(lo, g.s); hi = std::max(hi, g.e); }
        std::vector<JbbRec> hrec(hi - lo); std::vector<uint8_t> hkeep(hi - lo); std::vector<acc::Slot> hs(hi - lo);
        HIPCHK(hipMemcpy(hrec.data(), rec + lo, (size_t)(hi - lo) * sizeof(JbbRec), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(hkeep.data(), B.keep.p + ord0 + lo, (size_t)(hi - lo), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(hs.data(), slot + lo, (size_t)(hi - lo) * sizeof(acc::Slot), hipMemcpyDeviceToHost));
        std::vector<uint32_t> idx, ref; std::vector<int32_t> left;
        for (const AccBig& g : list) {
            idx.clear();
            for (uint32_t j = g.s; j < g.e; ++j) if (hkeep[j - lo] == 1) idx.push_back(j);
            std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return hrec[a - lo].rank < hrec[b - lo].rank; });       // hits: rank order
            ref.resize(idx.size()); left.resize(idx.size());
            for (size_t k = 0; k < idx.size(); ++k) { ref[k] = hrec[idx[k] - lo].ref_id; left[k] = hrec[idx[k] - lo].left; }
            const std::vector<uint32_t> iv = acc::sort_places(ref, left);
            const uint32_t base = hs[idx[0] - lo].out - hs[idx[0] - lo].place;
            for (size_t p = 0; p < iv.size(); ++p) {
                acc::Slot& sl = hs[idx[iv[p]] - lo];
                sl.place = (uint32_t)p; sl.out = base + (uint32_t)p;
                sl.flags &= ~(uint32_t)acc::SLOT_HAS_NEXT; sl.next_ref = 0; sl.next_left = 0;
                if (p + 1 < iv.size()) { sl.flags |= acc::SLOT_HAS_NEXT; sl.next_ref = ref[iv[p + 1]]; sl.next_left = left[iv[p + 1]]; }
            }
        }
        HIPCHK(hipMemcpy(slot + lo, hs.data(), (size_t)(hi - lo) * sizeof(acc::Slot), hipMemcpyHostToDevice));
    }
    // the settings on the device
    if (const int e = acc_grow(A.d_rg, A.rg.size() + 16)) return e;
    if (!A.rg.empty()) HIPCHK(hipMemcpyAsync(A.d_rg.p, A.rg.data(), A.rg.size(), hipMemcpyHostToDevice, c->stream));
    if (const int e = acc_grow(A.d_tid, A.tid.size() + 4)) return e;
    if (!A.tid.empty()) HIPCHK(hipMemcpyAsync(A.d_tid.p, A.tid.data(), A.tid.size() * 4, hipMemcpyHostToDevice, c->stream));
    acc::Cfg cfg{};
    cfg.library_type = A.library_type; cfg.rg = A.d_rg.p; cfg.rg_len = (uint32_t)A.rg.size(); cfg.tid_of_ref = A.d_tid.p; cfg.n_ref = (int32_t)A.tid.size();
    cfg.names = c->d_contig_names; cfg.name_off = c->d_contig_name_off;
    acc::mapq_table(cfg.mapq);
    hipLaunchKernelGGL(thj_k_acc_plan, acc_grid(n), dim3(256), 0, c->stream, r.infl, r.loc, (const uint32_t*)kept, (const acc::Slot*)slot, n, cfg, size_out, counters, in_bytes);
    thj_scan::exclusive_sum<uint32_t, unsigned long long>(c->stream, size_out, off, (int64_t)n_out + 1, c->d_sort_tmp);
    HIPCHK(hipGetLastError());
    unsigned long long total = 0, h_in = 0;
    HIPCHK(hipMemcpyAsync(h_cnt, counters, sizeof h_cnt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&total, off + n_out, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&h_in, in_bytes, 8, hipMemcpyDeviceToHost, c->stream));
    if (n_out) HIPCHK(hipMemcpyAsync(rec_size, size_out, (size_t)n_out * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (h_cnt[ACC_LOUD]) { thj_set_error("thj_juncbed_report_bam: %s", acc::loud_text(h_cnt[ACC_LOUD])); return THJ_EINVAL; }
    if (const int e = thj_bam_stream_reserve(c, (size_t)c->bam_bytes + (size_t)total + 64)) return e;
    if (n_out) {
        const int64_t blocks = (n + 3) / 4;
        hipLaunchKernelGGL(thj_k_acc_write, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, c->stream, r.infl, r.loc, (const uint32_t*)kept, (const acc::Slot*)slot, n, cfg,
                           (const unsigned long long*)off, c->d_bam + c->bam_bytes);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    c->bam_bytes += (int64_t)total;
    ++A.replayed; A.replayed_records += n;
    A.in_bytes += (int64_t)h_in; A.out_bytes += (int64_t)total;
    if (getenv("THJ_ACCEPTED_BYTES")) fprintf(stderr, "[accepted] piece %zu: %u records, %llu input record bytes read, %llu bytes written (all pieces so far: %lld + %lld)\n",
                                              A.replayed, n_out, h_in, total, (long long)A.in_bytes, (long long)A.out_bytes);
    *n_records = n_out; *total_bytes = c->bam_bytes;
    return THJ_OK;
}

// accepted_hits.bam for graded inserts (print_sam_for_pair and the sides that go alone): see include/thj.h
extern "C" int thj_juncbed_report_pairs_bam(thj_ctx* c, const uint8_t* left_recs, const int64_t* left_off, int64_t n_left, const uint8_t* right_recs, const int64_t* right_off,
                                            int64_t n_right, uint32_t* rec_size, int64_t rec_cap, int64_t* n_records, int64_t* total_bytes) {
    if (!c || n_left < 0 || n_right < 0 || (n_left > 0 && (!left_recs || !left_off)) || (n_right > 0 && (!right_recs || !right_off)) || rec_cap < 0 || !n_records || !total_bytes) {
        thj_set_error("thj_juncbed_report_pairs_bam: bad argument"); return THJ_EINVAL;
    }
    HIPCHK(hipSetDevice(c->device));
    JbState& S = c->jb; JbState::Accepted& A = S.acc;
    *n_records = 0; *total_bytes = 0;
    if (!A.on || !A.pairs || !S.pair.on) { thj_set_error("thj_juncbed_report_pairs_bam: the pass was not armed (thj_juncbed_collect_accepted_pairs and thj_juncbed_pair_alignments between the reset and the first add)"); return THJ_ESTATE; }
    if (!A.chosen) { thj_set_error("thj_juncbed_report_pairs_bam: no choice has been made yet (thj_juncbed_finish first)"); return THJ_ESTATE; }
    int64_t added = 0;
    for (const auto& pc : A.pcalls) added += pc.n_left + pc.n_right;
    if (added != S.records) { thj_set_error("thj_juncbed_report_pairs_bam: records were added by other calls than thj_juncbed_add_pairs[_seq]: only those can be replayed"); return THJ_ESTATE; }
    if (A.replayed >= A.pcalls.size()) { thj_set_error("thj_juncbed_report_pairs_bam: every add call of this consensus has been replayed already (%zu)", A.pcalls.size()); return THJ_ESTATE; }
    if (!c->d_contig_names || c->n_contig_names != c->n_contigs) { thj_set_error("thj_juncbed_report_pairs_bam: the context holds no names for the genome's %d contigs (thj_bam_contig_names_upload)", (int)c->n_contigs); return THJ_ESTATE; }
    const JbState::Accepted::PCall pc = A.pcalls[A.replayed];
    if (n_left != pc.n_left || n_right != pc.n_right) {
        thj_set_error("thj_juncbed_report_pairs_bam: %s (call %zu: %lld left and %lld right records, its add call %lld and %lld)", acc::loud_text(acc::LOUD_ORDER), A.replayed,
                      (long long)n_left, (long long)n_right, (long long)pc.n_left, (long long)pc.n_right);
        return THJ_EINVAL;
    }
    const int64_t n = n_left + n_right, ng = pc.n_ins;
    const bool first = A.replayed == 0, count_only = rec_size == nullptr;
    auto done = [&](int64_t n_out, int64_t bytes) {
        if (!count_only) { if (first) c->bam_bytes = 0; c->bam_bytes += bytes; ++A.replayed; A.replayed_records += n; A.out_bytes += bytes; }
        *n_records = n_out; *total_bytes = count_only ? bytes : c->bam_bytes;
        return THJ_OK;
    };
    if (n == 0 || ng == 0) return done(0, 0);
    // every record lies where its offsets say, behind a block_size field that says the same
    const size_t left_bytes = n_left ? (size_t)left_off[n_left] : 0, right_at = (left_bytes + 3) & ~(size_t)3, right_bytes = n_right ? (size_t)right_off[n_right] : 0;
    for (int side = 0; side < 2; ++side) {
        const uint8_t* r = side ? right_recs : left_recs; const int64_t* off = side ? right_off : left_off; const int64_t m = side ? n_right : n_left;
        for (int64_t i = 0; i < m; ++i) {
            const int64_t len = off[i + 1] - off[i];
            if ((i == 0 && off[0] != 0) || len < 36 || len > (1ll << 28) || (int64_t)acc::rd32(r + off[i]) + 4 != len) {
                thj_set_error("thj_juncbed_report_pairs_bam: %s (%s record %lld)", acc::loud_text(acc::LOUD_MALFORMED), side ? "right" : "left", (long long)i); return THJ_EINVAL;
            }
        }
    }
    // (src and the caller's records are the sources of asynchronous copies below: src is declared before the two scratch blocks, whose
    // destructors make the stream idle first -- on every way out, the early returns included -- and only then is src destroyed and the call over)
    std::vector<unsigned long long> src((size_t)n);
    {
        int64_t il = 0, ir = 0; size_t r = 0;
        for (int64_t g = 0; g < ng; ++g) {
            const uint32_t nl = A.p_nlr[2 * (size_t)(pc.first_ins + g)], nr = A.p_nlr[2 * (size_t)(pc.first_ins + g) + 1];
            if (il + nl > n_left || ir + nr > n_right || r + nl + nr > (size_t)n) { thj_set_error("thj_juncbed_report_pairs_bam: %s", acc::loud_text(acc::LOUD_ORDER)); return THJ_EINVAL; }
            for (uint32_t k = 0; k < nl; ++k) src[r++] = (unsigned long long)left_off[il++];
            for (uint32_t k = 0; k < nr; ++k) src[r++] = (unsigned long long)(right_at + (size_t)right_off[ir++]);
        }
        if (r != (size_t)n) { thj_set_error("thj_juncbed_report_pairs_bam: %s", acc::loud_text(acc::LOUD_ORDER)); return THJ_EINVAL; }
    }
    // how many output records every insert has, and where they begin
    const size_t g1 = (size_t)ng + 1;
    AccScratch sc1(c);
    if (const int rc = thj_dev_alloc(c, &sc1.p, ((g1 * 4 + 15) & ~(size_t)15) + g1 * 8 + 64)) return rc;
    unsigned long long* gbase = (unsigned long long*)sc1.p;
    uint32_t* gcnt = (uint32_t*)((char*)sc1.p + g1 * 8);
    HIPCHK(hipMemsetAsync(gcnt + ng, 0, 4, c->stream));
    if (const int rc = thj_accp_count(c, pc.first_ins, ng, gcnt)) return rc;
    if (const int e = ensure_sort_tmp(c, std::max(thj_scan::scratch_bytes((int64_t)g1, 8), (size_t)1 << 20))) return e;
    thj_scan::exclusive_sum<uint32_t, unsigned long long>(c->stream, gcnt, gbase, (int64_t)g1, c->d_sort_tmp);
    HIPCHK(hipGetLastError());
    unsigned long long n_out64 = 0;
    HIPCHK(hipMemcpyAsync(&n_out64, gbase + ng, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (n_out64 >= (1ull << 31)) { thj_set_error("thj_juncbed_report_pairs_bam: more than 2^31 - 1 output records in one call"); return THJ_EINVAL; }
    const int64_t n_out = (int64_t)n_out64;
    if (!count_only && n_out > rec_cap) { thj_set_error("thj_juncbed_report_pairs_bam: room for %lld record sizes, the call reports %lld records", (long long)rec_cap, (long long)n_out); return THJ_EINVAL; }
    if (n_out == 0) return done(0, 0);
    // scratch: offsets (n_out + 1), where every input record lies (n), the output records, their sizes (n_out + 1), the lists for the host, the
    // counters, the input records themselves
    const size_t o1 = (size_t)n_out + 1, big_cap = (size_t)n_out / (acc::SORT_BY_COUNTING + 1) + 1;
    const size_t b_off = o1 * 8, b_src = (size_t)n * 8, b_out = ((size_t)n_out * sizeof(AccPairOut) + 15) & ~(size_t)15, b_size = (o1 * 4 + 15) & ~(size_t)15,
                 b_big = (big_cap * sizeof(AccPairBig) + 15) & ~(size_t)15, b_raw = ((right_at + right_bytes + 3) & ~(size_t)3) + 16;
    AccScratch sc2(c);
    if (const int rc = thj_dev_alloc(c, &sc2.p, b_off + b_src + b_out + b_size + b_big + 64 + b_raw)) return rc;
    char* d = (char*)sc2.p;
    unsigned long long *off = (unsigned long long*)d, *src_off = (unsigned long long*)(d + b_off);
    AccPairOut* outs = (AccPairOut*)(d + b_off + b_src);
    uint32_t* size_out = (uint32_t*)((char*)outs + b_out);
    AccPairBig* big = (AccPairBig*)((char*)size_out + b_size);
    unsigned int* counters = (unsigned int*)((char*)big + b_big);
    uint8_t* raw = (uint8_t*)counters + 64;
    HIPCHK(hipMemsetAsync(counters, 0, 64, c->stream));
    HIPCHK(hipMemsetAsync(size_out + n_out, 0, 4, c->stream));
    HIPCHK(hipMemsetAsync(raw, 0, b_raw, c->stream));
    HIPCHK(hipMemcpyAsync(src_off, src.data(), b_src, hipMemcpyHostToDevice, c->stream));
    if (left_bytes) HIPCHK(hipMemcpyAsync(raw, left_recs, left_bytes, hipMemcpyHostToDevice, c->stream));
    if (right_bytes) HIPCHK(hipMemcpyAsync(raw + right_at, right_recs, right_bytes, hipMemcpyHostToDevice, c->stream));
    if (const int rc = thj_accp_layout(c, pc.first_ins, ng, gbase, outs, big, (uint32_t)big_cap, &counters[ACC_BIG])) return rc;
    unsigned int h_cnt[ACC_N_COUNTERS];
    HIPCHK(hipMemcpyAsync(h_cnt, counters, sizeof h_cnt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                    // (src was a copy's source)
    if (h_cnt[ACC_BIG]) {
        // lists of more than 16 entries: std::sort itself, on the sequence the reference sorts (best_hits' right records; a read's hits) with its comparator
        const size_t nb = h_cnt[ACC_BIG];
        if (nb > big_cap) { thj_set_error("thj_juncbed_report_pairs_bam: more long lists than records allow"); return THJ_EINVAL; }
        std::vector<AccPairBig> list(nb);
        HIPCHK(hipMemcpy(list.data(), big, nb * sizeof(AccPairBig), hipMemcpyDeviceToHost));
        std::vector<AccPairOut> in_hits, sorted;
        std::vector<uint32_t> ref; std::vector<int32_t> left;
        for (const AccPairBig& g : list) {
            const uint32_t w = g.pairs ? 2u : 1u, m = g.n / w;
            if ((uint64_t)g.base + g.n > (uint64_t)n_out || m * w != g.n) { thj_set_error("thj_juncbed_report_pairs_bam: a long list outside the output records"); return THJ_EINVAL; }
            in_hits.resize(g.n); sorted.resize(g.n); ref.resize(m); left.resize(m);
            HIPCHK(hipMemcpy(in_hits.data(), outs + g.base, (size_t)g.n * sizeof(AccPairOut), hipMemcpyDeviceToHost));
            for (uint32_t k = 0; k < m; ++k) { ref[k] = in_hits[(size_t)w * k].slot.ref_id; left[k] = in_hits[(size_t)w * k].left; }
            const std::vector<uint32_t> iv = acc::sort_places(ref, left);
            for (uint32_t p = 0; p < m; ++p)
                for (uint32_t x = 0; x < w; ++x) {
                    AccPairOut o = in_hits[(size_t)w * iv[p] + x];
                    o.slot.place = p; o.slot.out = g.base + w * p + x;
                    o.slot.flags &= ~(uint32_t)acc::SLOT_HAS_NEXT; o.slot.next_ref = 0; o.slot.next_left = 0;
                    if (p + 1 < m) { const AccPairOut& nx = in_hits[(size_t)w * iv[p + 1] + x]; o.slot.flags |= acc::SLOT_HAS_NEXT; o.slot.next_ref = nx.slot.ref_id; o.slot.next_left = nx.left; }
                    sorted[(size_t)w * p + x] = o;
                }
            HIPCHK(hipMemcpy(outs + g.base, sorted.data(), (size_t)g.n * sizeof(AccPairOut), hipMemcpyHostToDevice));
        }
    }
    // the settings on the device
    if (const int e = acc_grow(A.d_rg, A.rg.size() + 16)) return e;
    if (!A.rg.empty()) HIPCHK(hipMemcpyAsync(A.d_rg.p, A.rg.data(), A.rg.size(), hipMemcpyHostToDevice, c->stream));
    if (const int e = acc_grow(A.d_tid, A.tid.size() + 4)) return e;
    if (!A.tid.empty()) HIPCHK(hipMemcpyAsync(A.d_tid.p, A.tid.data(), A.tid.size() * 4, hipMemcpyHostToDevice, c->stream));
    acc::Cfg cfg{};
    cfg.library_type = A.library_type; cfg.rg = A.d_rg.p; cfg.rg_len = (uint32_t)A.rg.size(); cfg.tid_of_ref = A.d_tid.p; cfg.n_ref = (int32_t)A.tid.size();
    cfg.names = c->d_contig_names; cfg.name_off = c->d_contig_name_off;
    acc::mapq_table(cfg.mapq);
    hipLaunchKernelGGL(thj_k_accp_plan, acc_grid(n_out), dim3(256), 0, c->stream, (const uint8_t*)raw, (const unsigned long long*)src_off, (uint32_t)pc.first_rec, (const AccPairOut*)outs,
                       n_out, cfg, size_out, counters);
    if (const int e = ensure_sort_tmp(c, std::max(thj_scan::scratch_bytes((int64_t)o1, 8), (size_t)1 << 20))) return e;
    thj_scan::exclusive_sum<uint32_t, unsigned long long>(c->stream, size_out, off, (int64_t)o1, c->d_sort_tmp);
    HIPCHK(hipGetLastError());
    unsigned long long total = 0;
    HIPCHK(hipMemcpyAsync(h_cnt, counters, sizeof h_cnt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&total, off + n_out, 8, hipMemcpyDeviceToHost, c->stream));
    if (!count_only) HIPCHK(hipMemcpyAsync(rec_size, size_out, (size_t)n_out * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (h_cnt[ACC_LOUD]) { thj_set_error("thj_juncbed_report_pairs_bam: %s", acc::loud_text(h_cnt[ACC_LOUD], true)); return THJ_EINVAL; }
    if (count_only) return done(n_out, (int64_t)total);
    const int64_t at = first ? 0 : c->bam_bytes;
    if (first) c->bam_bytes = 0;
    if (const int e = thj_bam_stream_reserve(c, (size_t)at + (size_t)total + 64)) return e;
    const int64_t blocks = (n_out + 3) / 4;
    hipLaunchKernelGGL(thj_k_accp_write, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, c->stream, (const uint8_t*)raw, (const unsigned long long*)src_off, (uint32_t)pc.first_rec,
                       (const AccPairOut*)outs, n_out, cfg, (const unsigned long long*)off, c->d_bam + at);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return done(n_out, (int64_t)total);
}
