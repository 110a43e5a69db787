// thj_unmapped.hip -- unmapped_left_0.bam / unmapped_right_0.bam and the align-summary counters on the device (thj_juncbed_collect_unmapped,
// thj_juncbed_read_numbers, thj_juncbed_report_unmapped_bam, thj_juncbed_align_stats): after thj_juncbed_finish has chosen what every read and
// every insert reports, the reads files are walked piece by piece and every read is decided on its own -- written as GetReadProc::writeUnmapped
// writes it, or not, and counted into SAlignStats' fifteen counters.  The decisions and the record: thj_unmapped_core.h.
//
// What the finish leaves (JbState::Unmapped): read_best_alignments' code of every read at its first record (thj_k_jbb_cap), the word of every
// insert (thj_k_jbp_settle), and the read numbers in rising order -- per record for single-end input, so that a lower bound lands on a read's
// first record, per insert when inserts are graded.
// Per piece of a reads file (inflated and walked by thj_ingest_reads_walk):
//   thj_k_um_plan    a lane per record: number, FLAG, ZT, ZN; the numbers rise strictly (against the record before, the piece before); a
//                    binary search for the read's group / insert; um::decide -> written or not, its size, its counters.  Whole waves walk
//                    together: every counter is summed over the wave (a ballot) before lane 0 adds it once.
//   (scans)          written flags -> the records' places, sizes -> offsets
//   thj_k_um_sizes   the written records' sizes, densely, for the host's cut into BGZF members
//   thj_k_um_write   a WAVE per written record: um::emit with the wave's sink -- the header words by lane 0; QNAME, a forward SEQ and a QUAL
//                    without 0xff bytes as WaveSink's aligned-dword copies; a 0x10 record's SEQ and QUAL a lane per output byte
// The add calls number their reads as they go: thj_k_um_numbers reads the QNAMEs of a piece's kept records (thj_juncbed_add_bam), host arrays
// wait for thj_juncbed_read_numbers.
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
#include "thj_unmapped_core.h"
#include "thj_wave_sink.h"

namespace {

enum { UM_LOUD, UM_FOUND, UM_STAT0, UM_N_COUNTERS = UM_STAT0 + um::N_STATS + 1 };      // (an even number of words)

__device__ __forceinline__ const uint8_t* um_rec_at(const uint8_t* infl, uint32_t loc) { return infl + ((size_t)(loc >> 16) << 16) + (loc & 0xFFFFu); }

// thj_juncbed_add_bam: num[i] = the number of kept record i's read.  A read's records follow each other under one read_idx; where a new read
// begins its number must be above the one before (prev: the last number of the calls before, 0 = none)
__global__ __launch_bounds__(256) void thj_k_um_numbers(const uint8_t* __restrict__ infl, const uint32_t* __restrict__ loc, const thj_aln* __restrict__ aln, int64_t n, u64 prev,
                                                        u64* __restrict__ num, unsigned int* loud) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t* p = um_rec_at(infl, loc[i]);
        uint64_t v = 0;
        uint32_t bad = 0;
        if (!um::parse_number(p + 4, acc::rd32(p), v)) bad = um::LOUD_QNAME;
        else if (v == 0u) bad = um::LOUD_ZERO;
        else if (i == 0 || aln[i].read_idx != aln[i - 1].read_idx) {
            uint64_t pv = prev;
            if (i > 0) { const uint8_t* q = um_rec_at(infl, loc[i - 1]); if (!um::parse_number(q + 4, acc::rd32(q), pv)) pv = 0; }
            if (v <= pv) bad = um::LOUD_ORDER;
        }
        num[i] = v;
        if (bad) atomicOr(loud, bad);
    }
}

// what the finish kept.  num[0 .. n_num): single-end per record, paired per insert (ins / iword beside it)
struct UmTables { const u64* num; int64_t n_num; const uint8_t* code; int64_t n_code; const JbpIns* ins; const uint32_t* iword; };

__global__ __launch_bounds__(256) void thj_k_um_plan(const uint8_t* __restrict__ infl, const uint32_t* __restrict__ loc, int64_t n, um::Run run, uint32_t side, u64 prev, UmTables t,
                                                     uint32_t* __restrict__ kept, uint32_t* __restrict__ size, unsigned int* counters) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, n_iter = (n + stride - 1) / stride;
    for (int64_t it = 0; it < n_iter; ++it) {
        const int64_t i = it * stride + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        uint32_t cnt = 0, loud = 0;
        bool met = false;
        if (i < n) {
            const uint8_t* p = um_rec_at(infl, loc[i]);
            um::Read r;
            um::parse(p + 4, acc::rd32(p), r);
            loud = r.loud;
            uint32_t wr = 0, sz = 0;
            if (!loud) {
                uint64_t pv = prev;                             // (a record before that does not parse raises its own flag)
                if (i > 0) { const uint8_t* q = um_rec_at(infl, loc[i - 1]); if (!um::parse_number(q + 4, acc::rd32(q), pv)) pv = 0; }
                if (r.number <= pv) loud = um::LOUD_ORDER;
            }
            if (!loud) {
                int64_t a = 0, b = t.n_num;
                while (a < b) { const int64_t m = (a + b) >> 1; if (t.num[m] < r.number) a = m + 1; else b = m; }
                const bool found = a < t.n_num && t.num[a] == r.number;
                uint32_t word = 0, code = 0;
                if (found && !run.paired) { code = t.code[a]; met = true; }
                if (found && run.paired) {
                    word = t.iword[a];
                    met = (word & (side ? um::W_HAS_R : um::W_HAS_L)) != 0u;
                    const int64_t first = (int64_t)t.ins[a].first + (side ? (int64_t)t.ins[a].nl : 0);
                    if (met && first < t.n_code) code = t.code[first];
                }
                const um::Decision d = um::decide(run, side, found, word, code, r.zt, r.matenum);
                loud = d.loud;
                if (!loud) { cnt = d.counters; wr = d.write; sz = wr ? um::record_size(r) : 0u; }
            }
            kept[i] = wr; size[i] = sz;
        }
        if (loud) atomicOr(&counters[UM_LOUD], loud);
        const unsigned long long m_met = __ballot(met && !loud);
        if (lane == 0 && m_met) atomicAdd(&counters[UM_FOUND], (unsigned int)__popcll(m_met));
        for (int k = 0; k < um::N_STATS; ++k) {
            const unsigned long long m = __ballot((cnt >> k) & 1u);
            if (lane == 0 && m) atomicAdd(&counters[UM_STAT0 + k], (unsigned int)__popcll(m));
        }
    }
}

__global__ __launch_bounds__(256) void thj_k_um_sizes(const uint32_t* __restrict__ kept, const uint32_t* __restrict__ kb, const uint32_t* __restrict__ size, int64_t n, uint32_t* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        if (kept[i]) out[kb[i]] = size[i];
}

// the writing sink: WaveSink's copies, and the two spans writeUnmapped does not take over as they are
struct UmWaveSink : WaveSink {
    __device__ __forceinline__ void seq_fwd(uint32_t at, const uint8_t* src, uint32_t l) {
        copy(at, src, l >> 1);
        if ((l & 1u) && lane == 0u) o[at + (l >> 1)] = (uint8_t)(src[l >> 1] & 0xF0u);        // the spare nibble is 0
    }
    __device__ __forceinline__ void seq_rev(uint32_t at, const uint8_t* src, uint32_t l) { for (uint32_t j = lane; j < (l + 1u) >> 1; j += 64u) o[at + j] = um::revcomp_byte(src, l, j); }
    __device__ __forceinline__ void qual(uint32_t at, const uint8_t* src, uint32_t l, bool rev) {
        bool ff = false;
        if (!rev) for (uint32_t j = lane; j < l; j += 64u) ff |= src[j] == 0xFFu;
        if (!rev && !__any((int)ff)) { copy(at, src, l); return; }
        for (uint32_t j = lane; j < l; j += 64u) o[at + j] = um::qual_byte(src[rev ? l - 1u - j : j]);
    }
};

__global__ __launch_bounds__(256) void thj_k_um_write(const uint8_t* __restrict__ infl, const uint32_t* __restrict__ loc, const uint32_t* __restrict__ kept,
                                                      const unsigned long long* __restrict__ off, int64_t n, uint8_t* out) {
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t i = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < n; i += waves) {
        if (!kept[i]) continue;
        const uint8_t* p = um_rec_at(infl, loc[i]);
        um::Read r;
        um::parse(p + 4, acc::rd32(p), r);
        UmWaveSink sink;
        sink.o = out + off[i]; sink.lane = lane;
        (void)um::emit(p + 4, r, sink);
    }
}

struct UmScratch {
    thj_ctx* c; void* p = nullptr;
    explicit UmScratch(thj_ctx* c_) : c(c_) {}  UmScratch(const UmScratch&) = delete;
    ~UmScratch() { if (!p) return; (void)hipStreamSynchronize(c->stream); thj_dev_release(c, p); }
};
// a list that grows keeps its first `keep` entries (the stream is idle)
template <class T>
int um_grow(DevBuf<T>& b, int64_t keep, int64_t need) {
    if (need <= b.cap) return THJ_OK;
    const int64_t ncap = need + need / 4 + 4096;
    T* n = nullptr; HIPCHK(hipMalloc((void**)&n, (size_t)ncap * sizeof(T)));
    if (b.p && keep) HIPCHK(hipMemcpy(n, b.p, (size_t)keep * sizeof(T), hipMemcpyDeviceToDevice));
    (void)hipFree(b.p); b.p = n; b.cap = ncap;
    return THJ_OK;
}
dim3 um_grid(int64_t n) { const int64_t b = (n + 255) / 256; return dim3((unsigned)(b > 4096 ? 4096 : b < 1 ? 1 : b)); }

}  // namespace

extern "C" int thj_juncbed_collect_unmapped(thj_ctx* c, int32_t on, int32_t max_report_intron) {
    if (!c) { thj_set_error("null ctx"); return THJ_EINVAL; }
    if (on && max_report_intron < 0) { thj_set_error("thj_juncbed_collect_unmapped: bad argument (max_report_intron >= 0)"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    if (!c->jb.junc.tab.cap) { const int rc = thj_juncbed_reset_async(c); if (rc) return rc; }
    if (c->jb.records) { thj_set_error("thj_juncbed_collect_unmapped: records were added already (call it between reset and the first add)"); return THJ_ESTATE; }
    JbState::Unmapped& U = c->jb.um;
    U.reset();
    if (!on) return THJ_OK;
    if (!c->jb.best.on) { thj_set_error("thj_juncbed_collect_unmapped: best alignments are not being chosen (thj_juncbed_best_alignments first): which reads are unmapped is that choice"); return THJ_ESTATE; }
    U.max_report_intron = max_report_intron; U.on = true;
    return THJ_OK;
}

int thj_um_add_ok(thj_ctx* c, const char* who) {
    if (c->jb.um.on && c->jb.um.pending) { thj_set_error("%s: the unmapped reads are being collected and the add call before still waits for its read numbers (thj_juncbed_read_numbers)", who); return THJ_ESTATE; }
    return THJ_OK;
}

void thj_um_added(thj_ctx* c, int64_t n_units, bool numbered, const uint32_t* runs, int64_t has_l, int64_t has_r) {
    JbState::Unmapped& U = c->jb.um;
    U.n_has[0] += has_l; U.n_has[1] += has_r;
    if (numbered) { U.n_num = c->jb.records; U.last = U.cand_last; return; }
    U.pending = n_units;
    U.runs.clear();
    if (runs) { U.runs.assign(runs, runs + n_units); int64_t recs = 0; for (uint32_t x : U.runs) recs += x; U.pending_first = c->jb.records - recs; }
    else U.pending_first = c->jb.pair.n_ins - n_units;
}

int thj_um_numbers_bam(thj_ctx* c, const thj_reported_recs* r) {
    JbState::Unmapped& U = c->jb.um;
    const int64_t n = r->n, ord0 = c->jb.records;
    if (U.n_num != ord0) { thj_set_error("thj_juncbed_add_bam: the unmapped reads are being collected and %lld records of earlier add calls have no read numbers", (long long)(ord0 - U.n_num)); return THJ_ESTATE; }
    HIPCHK(hipStreamSynchronize(c->stream));
    if (const int e = um_grow(U.num, U.n_num, ord0 + n)) return e;
    UmScratch sc(c);
    if (const int rc = thj_dev_alloc(c, &sc.p, 64)) return rc;
    unsigned int* d_loud = (unsigned int*)sc.p;
    HIPCHK(hipMemsetAsync(d_loud, 0, 4, c->stream));
    hipLaunchKernelGGL(thj_k_um_numbers, um_grid(n), dim3(256), 0, c->stream, r->infl, r->loc, (const thj_aln*)r->recs, n, U.last, U.num.p + ord0, d_loud);
    HIPCHK(hipGetLastError());
    unsigned int loud = 0; u64 last = 0;
    HIPCHK(hipMemcpyAsync(&loud, d_loud, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&last, U.num.p + ord0 + n - 1, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (loud) { thj_set_error("thj_juncbed_add_bam: the unmapped reads are being collected: %s (the alignments' QNAMEs are the read numbers)", um::loud_text(loud)); return THJ_EINVAL; }
    U.cand_last = last;
    return THJ_OK;
}

extern "C" int thj_juncbed_read_numbers(thj_ctx* c, const uint64_t* numbers, int64_t n) {
    if (!c || n < 0 || (n > 0 && !numbers)) { thj_set_error("thj_juncbed_read_numbers: bad argument"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    JbState::Unmapped& U = c->jb.um;
    if (!U.on) { thj_set_error("thj_juncbed_read_numbers: the unmapped reads are not being collected (thj_juncbed_collect_unmapped between the reset and the first add)"); return THJ_ESTATE; }
    if (!U.pending) { if (n == 0) return THJ_OK; thj_set_error("thj_juncbed_read_numbers: no add call waits for read numbers (right after thj_juncbed_add_records[_seq] or thj_juncbed_add_pairs[_seq])"); return THJ_ESTATE; }
    const bool pairs = U.runs.empty();
    if (n != U.pending) { thj_set_error("thj_juncbed_read_numbers: %lld numbers, the add call before has %lld %s", (long long)n, (long long)U.pending, pairs ? "inserts" : "reads"); return THJ_EINVAL; }
    u64 prev = U.last;
    for (int64_t k = 0; k < n; ++k) {
        if (numbers[k] == 0u) { thj_set_error("thj_juncbed_read_numbers: %s (entry %lld)", um::loud_text(um::LOUD_ZERO), (long long)k); return THJ_EINVAL; }
        if (numbers[k] <= prev) { thj_set_error("thj_juncbed_read_numbers: %s (entry %lld: %llu after %llu)", um::loud_text(um::LOUD_ORDER), (long long)k, (unsigned long long)numbers[k], (unsigned long long)prev); return THJ_EINVAL; }
        prev = numbers[k];
    }
    std::vector<u64> flat;
    if (pairs) flat.assign(numbers, numbers + n);
    else for (int64_t k = 0; k < n; ++k) flat.insert(flat.end(), (size_t)U.runs[(size_t)k], (u64)numbers[k]);
    const int64_t at = U.pending_first, m = (int64_t)flat.size();
    if (at != U.n_num) { thj_set_error("thj_juncbed_read_numbers: earlier add calls have no read numbers"); return THJ_ESTATE; }
    HIPCHK(hipStreamSynchronize(c->stream));
    if (const int e = um_grow(U.num, U.n_num, at + m)) return e;
    HIPCHK(hipMemcpy(U.num.p + at, flat.data(), (size_t)m * sizeof(u64), hipMemcpyHostToDevice));
    U.n_num = at + m; U.last = prev; U.pending = 0; U.runs.clear();
    return THJ_OK;
}

extern "C" int thj_juncbed_report_unmapped_bam(thj_ctx* c, int32_t side, const thj_bam_piece* piece, int32_t more_follows, int64_t* n_records, uint32_t* resume_member,
                                               uint32_t* resume_skip, uint32_t* rec_size, int64_t rec_cap, int64_t* total_bytes) {
    if (!c || side < 0 || side > 1 || !piece || piece->comp_bytes < 0 || (piece->comp_bytes > 0 && !piece->comp) || !n_records || !resume_member || !resume_skip || rec_cap < 0 ||
        !total_bytes) { thj_set_error("thj_juncbed_report_unmapped_bam: bad argument"); return THJ_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    JbState& S = c->jb; JbState::Unmapped& U = S.um;
    *n_records = 0; *resume_member = 0; *resume_skip = 0; *total_bytes = 0;
    if (!U.on) { thj_set_error("thj_juncbed_report_unmapped_bam: the pass was not armed (thj_juncbed_collect_unmapped between the reset and the first add)"); return THJ_ESTATE; }
    if (!U.chosen) { thj_set_error("thj_juncbed_report_unmapped_bam: no choice has been made yet (thj_juncbed_finish first)"); return THJ_ESTATE; }
    const bool paired = S.pair.on, count_only = rec_size == nullptr;
    if (side == 1 && !paired) { thj_set_error("thj_juncbed_report_unmapped_bam: bad argument (side 1 is the right reads file of a consensus whose inserts are graded)"); return THJ_EINVAL; }
    const int64_t units = paired ? S.pair.n_ins : S.records;
    if (U.pending || U.n_num != units) { thj_set_error("thj_juncbed_report_unmapped_bam: %lld %s of the consensus have no read numbers (thj_juncbed_read_numbers after every host-array add call)",
                                                       (long long)(units - U.n_num), paired ? "inserts" : "records"); return THJ_ESTATE; }
    if (U.done[side]) { thj_set_error("thj_juncbed_report_unmapped_bam: the last piece of this side's reads file has been reported already"); return THJ_ESTATE; }
    thj_reads_recs r;
    if (const int rc = thj_ingest_reads_walk(c, piece, &r)) return rc;
    const int64_t n = r.n;
    auto done = [&](int64_t n_out, int64_t bytes, const unsigned int* h_cnt, u64 last) {
        if (!count_only) {
            if (U.pieces[side] == 0) c->bam_bytes = 0;          // the first piece of a side opens the stream
            c->bam_bytes += bytes; ++U.pieces[side];
            if (h_cnt) { U.found[side] += h_cnt[UM_FOUND]; for (int k = 0; k < um::N_STATS; ++k) U.stats[k] += h_cnt[UM_STAT0 + k]; }
            if (last) U.last_read[side] = last;
            if (!more_follows) U.done[side] = true;
        }
        *n_records = n_out; *total_bytes = count_only ? bytes : c->bam_bytes;
        *resume_member = r.n_members; *resume_skip = 0;        // every record stands alone: a piece is taken whole
        return THJ_OK;
    };
    if (n == 0) return done(0, 0, nullptr, 0);
    if (n >= (1ll << 31)) { thj_set_error("thj_juncbed_report_unmapped_bam: more than 2^31 - 1 records in one piece"); return THJ_EINVAL; }
    // scratch: offsets (n + 1), [kept | kb | size | the written records' sizes] (n + 1 each), the counters
    const size_t n1 = (size_t)n + 1, b_u32 = (n1 * 4 + 15) & ~(size_t)15, b_off = n1 * 8;
    UmScratch scratch(c);
    if (const int rc = thj_dev_alloc(c, &scratch.p, b_off + 4 * b_u32 + UM_N_COUNTERS * 4 + 64)) return rc;
    char* d = (char*)scratch.p;
    unsigned long long* off = (unsigned long long*)d;
    uint32_t *kept = (uint32_t*)(d + b_off), *kb = (uint32_t*)((char*)kept + b_u32), *size = (uint32_t*)((char*)kb + b_u32), *csize = (uint32_t*)((char*)size + b_u32);
    unsigned int* counters = (unsigned int*)((char*)csize + b_u32);
    HIPCHK(hipMemsetAsync(counters, 0, UM_N_COUNTERS * 4, c->stream));
    HIPCHK(hipMemsetAsync(kept, 0, 3 * b_u32, c->stream));     // (kept, kb, size: the entry behind the last record stays 0)
    const um::Run run{(uint8_t)(paired ? 1 : 0), (uint8_t)(S.pair.mixed ? 1 : 0)};
    const UmTables t{U.num.p, U.n_num, U.code.p, S.records, paired ? S.pair.ins.p : nullptr, paired ? U.iword.p : nullptr};
    hipLaunchKernelGGL(thj_k_um_plan, um_grid(n), dim3(256), 0, c->stream, r.infl, r.loc, n, run, (uint32_t)side, U.last_read[side], t, kept, size, counters);
    if (const int e = ensure_sort_tmp(c, std::max(thj_scan::scratch_bytes((int64_t)n1, 8), (size_t)1 << 20))) return e;
    thj_scan::exclusive_sum<uint32_t, uint32_t>(c->stream, kept, kb, (int64_t)n1, c->d_sort_tmp);
    thj_scan::exclusive_sum<uint32_t, unsigned long long>(c->stream, size, off, (int64_t)n1, c->d_sort_tmp);
    hipLaunchKernelGGL(thj_k_um_sizes, um_grid(n), dim3(256), 0, c->stream, (const uint32_t*)kept, (const uint32_t*)kb, (const uint32_t*)size, n, csize);
    HIPCHK(hipGetLastError());
    unsigned int h_cnt[UM_N_COUNTERS];
    uint32_t n_out = 0, last_loc = 0;
    unsigned long long total = 0;
    HIPCHK(hipMemcpyAsync(h_cnt, counters, sizeof h_cnt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&n_out, kb + n, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&total, off + n, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&last_loc, r.loc + (n - 1), 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (h_cnt[UM_LOUD]) { thj_set_error("thj_juncbed_report_unmapped_bam: %s", um::loud_text(h_cnt[UM_LOUD])); return THJ_EINVAL; }
    if (count_only) return done((int64_t)n_out, (int64_t)total, nullptr, 0);
    if ((int64_t)n_out > rec_cap) { thj_set_error("thj_juncbed_report_unmapped_bam: room for %lld record sizes, the piece writes %u records", (long long)rec_cap, n_out); return THJ_EINVAL; }
    // the piece's last number, for the piece after it (the record parsed: no flag was raised)
    u64 last = 0;
    {
        uint8_t head[64];
        const uint8_t* p = r.infl + ((size_t)(last_loc >> 16) << 16) + (last_loc & 0xFFFFu);
        HIPCHK(hipMemcpy(head, p, 60, hipMemcpyDeviceToHost));      // block_size, the 32 fixed bytes, a QNAME of at most 19 bytes
        uint64_t v = 0;
        um::parse_number(head + 4, 56u, v);
        last = v;
    }
    const int64_t at = U.pieces[side] == 0 ? 0 : c->bam_bytes;
    if (U.pieces[side] == 0) c->bam_bytes = 0;
    if (const int e = thj_bam_stream_reserve(c, (size_t)at + (size_t)total + 64)) return e;
    if (n_out) {
        HIPCHK(hipMemcpyAsync(rec_size, csize, (size_t)n_out * 4, hipMemcpyDeviceToHost, c->stream));
        const int64_t blocks = (n + 3) / 4;
        hipLaunchKernelGGL(thj_k_um_write, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, c->stream, r.infl, r.loc, (const uint32_t*)kept, (const unsigned long long*)off, n,
                           c->d_bam + at);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return done((int64_t)n_out, (int64_t)total, h_cnt, last);
}

extern "C" int thj_juncbed_align_stats(thj_ctx* c, int64_t* stats) {
    if (!c || !stats) { thj_set_error("thj_juncbed_align_stats: bad argument"); return THJ_EINVAL; }
    JbState& S = c->jb; JbState::Unmapped& U = S.um;
    for (int k = 0; k < um::N_STATS; ++k) stats[k] = 0;
    if (!U.on) { thj_set_error("thj_juncbed_align_stats: the pass was not armed (thj_juncbed_collect_unmapped between the reset and the first add)"); return THJ_ESTATE; }
    if (!U.chosen) { thj_set_error("thj_juncbed_align_stats: no choice has been made yet (thj_juncbed_finish first)"); return THJ_ESTATE; }
    const int sides = S.pair.on ? 2 : 1;
    for (int s = 0; s < sides; ++s)
        if (!U.done[s]) { thj_set_error("thj_juncbed_align_stats: the %s reads file has not been reported to its end (thj_juncbed_report_unmapped_bam with more_follows == 0)", s ? "right" : "left"); return THJ_ESTATE; }
    for (int s = 0; s < sides; ++s)
        if (U.found[s] != U.n_has[s]) {
            thj_set_error("thj_juncbed_align_stats: %lld %s reads with alignments were met in no reads file (the reference warns \"Should never happen\" and goes on; this build does not guess)",
                          (long long)(U.n_has[s] - U.found[s]), s ? "right" : "left");
            return THJ_EINVAL;
        }
    for (int k = 0; k < um::N_STATS; ++k) stats[k] = U.stats[k];
    return THJ_OK;
}
