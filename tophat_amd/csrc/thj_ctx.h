// thj_ctx.h -- the context object shared by the translation units of libthj_hip.so (internal)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/thj.h"
#include "thj_core.h"
#include "thj_internal.h"
#include "thj_jbknown_core.h"

using thj::u64;

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e__ = (expr);                                                              \
        if (e__ != hipSuccess) {                                                              \
            thj_set_error("%s: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            return THJ_EHIP;                                                                  \
        }                                                                                     \
    } while (0)

// a span batch this library made (thj_span_batch_upload, thj_ingest_span_*): the API descriptor first, then what it owns
struct OwnedSpanBatch {
    thj_span_batch desc;
    void* ptrs[8];               // 0 seg_off, 1 hits, 2 read planes, 3 read lengths, 4 qualities, 5 hit heads,
                                 // 6 the reads' own (inflated) BAM records, 7 uint32 per row: where its record starts in [6]
    size_t reads_infl_bytes;     // size of [6]
};

// DevBuf: a device buffer that grows, pointer and capacity in elements
template <class T> struct DevBuf { T* p = nullptr; int64_t cap = 0; void release() { (void)hipFree(p); p = nullptr; cap = 0; } };
// junction consensus (thj_juncbed_impl.h and the two headers it includes), everything the pass owns.  JbStore: a hash table of `cap` slots -- u64
// columns, uint32 columns, counters; which: the JbLayout declared beside the table's struct.
struct JbStore { DevBuf<u64> w64; DevBuf<uint32_t> w32; DevBuf<unsigned long long> cnt; int64_t cap = 0; void release() { w64.release(); w32.release(); cnt.release(); cap = 0; } };
struct JbOcc; struct JbiOcc; struct JbfOcc; struct JbfUOcc; struct JbfJOcc; struct JbbRec; struct JbpIns; struct JbpCand;
struct JbState {
    int64_t want = 0, records = 0;              // thj_juncbed_configure's capacity; records added since the reset
    jbk::ReadFilter flt{};                      // thj_juncbed_read_filter; off after a reset
    // known: the annotated junctions (thj_juncbed_known_junctions), n_known sorted unique keys; none after a reset
    struct Junc { JbStore tab; DevBuf<u64> sorted; DevBuf<JbOcc> occ; int64_t occ_used = 0; DevBuf<u64> known; int64_t n_known = 0; std::vector<thj_juncstat> rows; } junc;
    // the indel sets reduced beside it when asked for (two tables side by side in one store), and the fusion set: grp = [group sizes | records
    // of the group the filter drops] per read of every add call
    struct Indel { bool on = false; JbStore tab; DevBuf<JbiOcc> occ; int64_t occ_used = 0; std::vector<thj_insstat> ins; std::vector<thj_juncstat> del; } indel;
    struct Fus { bool on = false; int32_t anchor = 20, mismatches = 2, multireads = 2; JbStore tab; DevBuf<uint32_t> grp; int64_t groups = 0;
                 DevBuf<JbfOcc> focc; DevBuf<JbfUOcc> uocc; DevBuf<JbfJOcc> jocc; std::vector<thj_fusstat> rows; } fus;
    // only each read's best alignments count (thj_juncbed_best_alignments): what is kept of every record added, the score keys of the junction
    // occurrences (as many as junc.occ holds), the keep flags the last finish wrote, the device counters and their last download
    struct Best { bool on = false; int32_t max_multihits = 20, suppress = 0, max_penalty = 6; DevBuf<JbbRec> rec; DevBuf<u64> skey; DevBuf<uint8_t> keep;
                  DevBuf<unsigned long long> cnt; int64_t counts[4] = {0, 0, 0, 0}; } best;
    // the reported alignments are written out afterwards (thj_juncbed_collect_accepted, thj_accepted.hip): what finish keeps for that beside
    // best.rec and best.keep -- the second pass's scores, per record the reporting reads before it (records + 1 entries), per reporting read
    // the generator's raw output for print_sam_for_single (device and host) -- the records of every thj_juncbed_add_bam call, and how far the
    // replay has come: calls replayed, records replayed.  chosen: a finish has filled them in.
    // pairs: armed by thj_juncbed_collect_accepted_pairs (inserts may be graded beside it)
    struct Accepted { bool on = false, chosen = false, pairs = false; int32_t library_type = 0; std::vector<uint8_t> rg; DevBuf<int32_t> score; DevBuf<uint32_t> before, draw;
                      std::vector<uint32_t> h_draw; std::vector<int64_t> calls; size_t replayed = 0; int64_t replayed_records = 0; DevBuf<uint8_t> d_rg;
                      std::vector<int32_t> tid; DevBuf<int32_t> d_tid;       // the output header's target of every contig
                      int64_t in_bytes = 0, out_bytes = 0;                   // what the write kernel has read and written since the reset
                      // beside graded inserts (thj_juncbed_pair_alignments; thj_juncbed_report_pairs_bam writes their records): what the finish
                      // used to throw away -- every insert's candidate list, its length, its flags (JBP_REPORTS, JBP_HAPPY), where its order lies
                      // when the host sorted it, the orders, per insert over the cap the word its bits begin at in the mask (~0: none), the
                      // mask.  The primary draw of an insert that reports pairs is draw[before[its first record]], as a read's is.  On the
                      // host: the records a side of every thj_juncbed_add_pairs call, and (nl, nr) of its inserts in visit order.
                      DevBuf<JbpCand> p_cand; DevBuf<uint32_t> p_gnk, p_gflags, p_order, p_mword, p_mask; DevBuf<u64> p_gbig;
                      struct PCall { int64_t n_left, n_right, first_rec, first_ins, n_ins; };
                      std::vector<PCall> pcalls; std::vector<uint32_t> p_nlr;
                      void release() { score.release(); before.release(); draw.release(); d_rg.release(); d_tid.release(); p_cand.release(); p_gnk.release(); p_gflags.release();
                                       p_order.release(); p_mword.release(); p_mask.release(); p_gbig.release(); } } acc;
    // inserts are graded (thj_juncbed_pair_alignments, thj_juncbed_pair_impl.h): the groups of every thj_juncbed_add_pairs call in visit order, how
    // many of them have both sides, the candidates their lists can hold at most, the lists that may go to the host for their sort (more than
    // 16 candidates) and those lists' candidates; per record the reported pairs it is in and its place in the reference's order of observation (the last finish wrote them); the device counters
    // and their last download
    struct Pair { bool on = false; int32_t mean = 200, sd = 20, fusion_min_dist = 10000000; bool mixed = false, discordant = false;
                  DevBuf<JbpIns> ins; int64_t n_ins = 0, n_both = 0, n_cand = 0, n_big = 0, n_bigcand = 0; DevBuf<uint32_t> pcnt, pprio;
                  DevBuf<unsigned long long> cnt; int64_t counts[5] = {0, 0, 0, 0, 0}; } pair;
    // the unmapped-read files and the align-summary counters (thj_juncbed_collect_unmapped, thj_unmapped.hip): what the finish keeps for them until
    // the next reset -- read_best_alignments' code of every read at its first record, the word of every insert (um::insert_word) -- and the read
    // numbers: per record (single-end: the binary search lands on a read's first record) or per insert (inserts graded), n_num of them.
    // pending: the reads / inserts of the last host-array add call, still without numbers (thj_juncbed_read_numbers), runs = their record counts.
    // last: the last number taken (cand_last: of a piece whose records are not counted yet).  n_has[side]: reads with an alignment group.  After the finish: per side the pieces reported, the reads with a group that were met, the
    // last number met, whether the side's last piece has been reported; the counters so far.
    struct Unmapped { bool on = false, chosen = false; int32_t max_report_intron = 0; DevBuf<u64> num; int64_t n_num = 0, pending = 0, pending_first = 0;
                      std::vector<uint32_t> runs; u64 last = 0, cand_last = 0; DevBuf<uint8_t> code; DevBuf<uint32_t> iword; int64_t n_has[2] = {0, 0};
                      int64_t pieces[2] = {0, 0}, found[2] = {0, 0}; u64 last_read[2] = {0, 0}; bool done[2] = {false, false}; int64_t stats[15] = {};
                      void reset() { on = chosen = false; n_num = pending = pending_first = 0; runs.clear(); last = cand_last = 0; n_has[0] = n_has[1] = 0; replay(); }
                      void replay() { for (int s = 0; s < 2; ++s) { pieces[s] = found[s] = 0; last_read[s] = 0; done[s] = false; } for (int64_t& x : stats) x = 0; }
                      void release() { num.release(); code.release(); iword.release(); } } um;
};

// coverage, butterfly and microexon searches (thj_covsearch_impl.h), everything they own
struct CovState {
    // what depends on the genome, and the genome it is sized for (cov_ensure): 8 bitmaps of n_blocks words each, named by cov_view; max(right) + 1
    // per contig
    int64_t n_blocks = 0; int32_t n_contigs = 0;
    DevBuf<u64> bits; DevBuf<int32_t> extent;
    unsigned long long* d_found = nullptr;      // [0] candidates a pairing pass found; [1] left sites listed / microexon candidates of a batch
    // a record per unmapped read: min(length, 32) and its first 32 bases as a 2-bit string (thj_cov_core.h: read_record); n_reads of them
    DevBuf<uint32_t> rec_len; DevBuf<u64> rec_seq; int64_t n_reads = 0;
    // the extension table made from the records (cov_build_table): offsets per seed with the scatter's cursors behind them, the entries by
    // seed, the Bloom filter over them (64-bit words) and its mask
    uint32_t* d_ext_off = nullptr; DevBuf<u64> ext_val; DevBuf<u64> filter; u64 filter_mask = 0;
    // the candidate list of a pairing pass, shared by the three searches: junction key and skip count, and a sibling of each for the cut's
    // sorts; one capacity.  No list yet: cap 0 and null pointers, and a pass into it only counts (cov_list_reserve, cov_list_settle)
    struct List {
        u64 *key = nullptr, *key2 = nullptr; uint32_t *skip = nullptr, *skip2 = nullptr; int64_t cap = 0;
        void release() { (void)hipFree(key); (void)hipFree(key2); (void)hipFree(skip); (void)hipFree(skip2); *this = List(); }
    } list;
    DevBuf<thj_mx_cand> mx_cand; int64_t n_mx_cand = 0;        // microexon search: candidate windows of the pass's reads
    int32_t min_intron = 0, max_intron = 0; bool pending = false;       // a coverage search launched (thj_covsearch_run_async) and not finished
    void release() {
        bits.release(); extent.release(); rec_len.release(); rec_seq.release(); ext_val.release(); filter.release(); list.release(); mx_cand.release();
        (void)hipFree(d_found); (void)hipFree(d_ext_off); *this = CovState();
    }
};

struct thj_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // the side streams for everything that runs beside the context's stream: [0] / [1] = the first / second batch of a pair call, in
    // stage 1 (SjPlan in thj_segjuncs.hip) and in stage 2 (span_run_common in thj_span.hip).  Two side streams, not one per chain: HIP
    // spreads streams over GPU_MAX_HW_QUEUES (4) hardware queues round robin, two streams on one queue run one after the other, and a
    // process has other streams too -- with ten streams the second side's chain of stage 1 sat behind the first side's (profiles/r05_e_timeline.txt)
    hipStream_t aux_stream[2] = {};
    // what the probe measured when it took side stream k: a spin kernel on it beside one on the context's stream and on every side stream
    // taken before, over a spin kernel alone (1.0 = fully beside each other, 2.0 = one queue shared); 0 = not measured.  aux_independent
    // = measured and below 1.5 (thj_ctx_stream_info, thj_streams.hip)
    double aux_ratio[2] = {0, 0}; bool aux_independent[2] = {false, false};
    // genome
    const u64* d_blocks = nullptr; bool own_blocks = false;
    uint32_t* d_contig_blk = nullptr; int32_t* d_contig_len = nullptr;
    std::vector<uint32_t> h_contig_blk; std::vector<int64_t> h_lens;
    int32_t n_contigs = 0; int64_t n_blocks = 0;
    // tables
    int64_t junc_cap = 0, indel_cap = 0;
    u64 *d_junc = nullptr, *d_del = nullptr, *d_ins_key = nullptr, *d_ins_val = nullptr;
    unsigned int* d_ovf = nullptr;
    unsigned long long* d_cnt = nullptr;
    // sorted outputs
    u64 *d_junc_sorted = nullptr, *d_del_sorted = nullptr, *d_ins_key_sorted = nullptr, *d_ins_val_sorted = nullptr;
    u64 *d_tmp_keys = nullptr, *d_tmp_vals = nullptr, *d_tmp_keys2 = nullptr;   // event lists (see set_insert) / insertion gather
    int64_t out_cap_junc = 0, out_cap_indel = 0;
    unsigned long long* d_out_n = nullptr;      // [3]
    unsigned long long* h_pinned = nullptr;     // [16] pinned staging
    void* d_sort_tmp = nullptr; size_t sort_tmp_bytes = 0;
    int64_t n_junc = 0, n_del = 0, n_ins = 0;
    hipEvent_t probe_ev = nullptr; bool probe_pending = false;            // insert counters on their way to h_pinned[32..]
    uint8_t* d_fus_ignore = nullptr; int64_t n_fus_ignore = 0;            // --fusion-ignore-chromosomes flags per ref id
    // stage 1's scratch of a batch in flight (SjGeom / SjPlan in thj_segjuncs.hip): two sets, one per batch of a pair call
    struct SjSet {
        uint32_t* d_rescue_list = nullptr; int64_t rescue_list_cap = 0;      // reads taking the mate-anchored rescue + per-workgroup counts (words)
        uint32_t* d_many = nullptr;                                          // reads with many hits of a launch (thj_k_segjuncs_shared): count, list
        void* d_lists = nullptr; size_t lists_cap = 0;                       // the flat kernels' task / rescue / general-read lists (thj_k_sj_flat) (bytes)
        int32_t* d_rescue_slots = nullptr;                                   // rescue outcomes of reads with many hits (thj_k_segjuncs_rescue)
        hipEvent_t ev_flat = nullptr, ev_side = nullptr;                     // thj_k_sj_flat done: the side stream starts; the side chain done: sj_join waits for it
    } sj_set[2];
    // long_spanning_reads (thj_span.hip)
    uint32_t* d_junc_bucket = nullptr; int64_t n_junc_buckets = 0;     // coarse index over d_span_junc (junc_range)
    u64* d_span_cat = nullptr;                                            // junction ++ deletion keys before their sort
    u64* d_span_junc = nullptr; int64_t n_span_junc = 0; int64_t cap_span_junc = 0;
    u64* d_span_ins_key = nullptr; uint32_t* d_span_ins_seq = nullptr; int64_t n_span_ins = 0; int64_t cap_span_ins = 0;
    void* d_huge_ws = nullptr; uint32_t* d_huge_list = nullptr; int huge_blocks = 0, huge_list_cap = 0;      // reads with too many joined alignments for a thread's array (thj_k_stitch_huge)
    void* d_span_fus = nullptr; int64_t n_span_fus = 0; int64_t cap_span_fus = 0;       // --fusion-search: the sorted .fusions list (thj_span_fusions_upload)
    void* d_aln_pool = nullptr; void* d_aln_sorted = nullptr; int64_t aln_cap = 0;
    u64* d_aln_keys = nullptr;
    unsigned long long* d_aln_count = nullptr; unsigned int* d_span_status = nullptr;
    int64_t n_alns = 0, n_ovf = 0, span_reads = 0, ovf_cap = 0;
    uint8_t* d_nrec = nullptr;
    std::vector<thj_aln> h_alns;
    // scratch of a batch in flight (SpanPlan in thj_span.hip): two sets, so that the two sides of a pass can run beside each other
    struct SpanSet { uint32_t* d_worklist = nullptr; int64_t worklist_cap = 0; void* d_ent = nullptr; int64_t ent_cap = 0; void* d_joined = nullptr; int64_t joined_cap = 0; uint32_t* d_defer = nullptr; int64_t defer_cap = 0; };
    SpanSet span_set[2]; int span_last_set = 0;
    // thj_span_tier0_pair_async ran the pair's tier 0 ahead of thj_span_run_pair_async (which then only does what is behind it)
    bool span_t0_pending = false; int64_t span_t0_n[2] = {0, 0}; hipEvent_t span_t0_prof[2][32] = {};
    hipEvent_t span_ev[10] = {};         // (its streams are aux_stream[0 .. 1])
    bool span_profile = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> span_prof_events;
    CovState cov;                               // coverage, butterfly and microexon searches (thj_covsearch_impl.h)
    // fusion search
    thj_fusion* d_fus = nullptr; unsigned long long* d_fus_count = nullptr; int64_t fus_cap = 0;
    hipEvent_t fus_probe_ev = nullptr; bool fus_probe_pending = false;      // the raw event count on its way to h_pinned[44] (the buffer grows ahead of it)
    std::vector<thj_fusion> h_fusions;
    thj_fusion* d_fus_out = nullptr; int64_t n_fus_out = 0;            // the reduced set on the device (Fusion::operator< order); null: only h_fusions holds it
    bool h_fus_stale = false;                                          // h_fusions not yet copied down from d_fus_out
    // batch arrays come and go once per shard / batch: hipMalloc and (synchronising) hipFree per array cost more than the
    // kernels of a small shard, so released blocks are kept and handed out again (thj_dev_alloc / thj_dev_release)
    struct DevBlock { void* p; size_t cap; bool used; };
    std::vector<DevBlock> dev_cache; size_t dev_cache_bytes = 0;
    // device-side ingest scratch (thj_ingest.hip)
    void* d_ing0 = nullptr; size_t ing_cap0 = 0; void* d_ing1 = nullptr; size_t ing_cap1 = 0;
    // the run's junction-db target table (thj_span_juncdb_upload): what the parse kernel resolves a spliced map's targets with
    thj_juncdb_target* d_juncdb = nullptr; int64_t n_juncdb = 0;
    // ... whether it holds a THJ_JUNCDB_FUS target, and the table's switch (thj_span_juncdb_fusion_contigs; every upload turns it off)
    bool juncdb_has_fus = false, juncdb_fusion_on = false;
    // the BAM writer's device side (thj_bamout.hip): the pass's encoded records, their offsets; the deflater's scratch
    uint8_t* d_bam = nullptr; size_t bam_cap = 0; int64_t bam_bytes = 0;
    void* d_bam_tmp = nullptr; size_t bam_tmp_cap = 0;
    uint8_t* d_contig_names = nullptr; uint32_t* d_contig_name_off = nullptr; uint32_t* d_contig_name_sorted = nullptr; int32_t n_contig_names = 0;    // XF:Z's contig names (thj_bam_contig_names_upload)
    void* d_infl_tmp = nullptr; size_t infl_tmp_cap = 0;                  // token streams of the two-kernel inflater
    JbState jb;                                 // junction consensus (thj_juncbed_impl.h)
    // multi-GPU exchange step pending a look at its gathered headers (thj_exchange_impl.h)
    struct thj_comm* xchg = nullptr;
    // profiling
    bool profile = false;
    bool serial_launch = false;                 // thj_profile_serial: no side streams
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
    std::vector<hipEvent_t> prof_all; std::vector<int> prof_sets;       // every event of prof_events once; the scratch set of each profiled launch
    std::vector<hipEvent_t> event_pool;
};
// a device buffer that only grows: the device idle first (a launch may still be using the smaller one), free, malloc, then the new
// capacity -- a hipMalloc that fails leaves the pointer null and the capacity 0.  The old contents are dead.  `cap` is in the caller's unit.
template <class T, class C>
static inline int grow_device_buffer(T*& ptr, C& cap, C new_cap, size_t bytes) {
    if (ptr) HIPCHK(hipDeviceSynchronize());
    (void)hipFree(ptr); ptr = nullptr; cap = 0;
    HIPCHK(hipMalloc((void**)&ptr, bytes));
    cap = new_cap;
    return THJ_OK;
}
// the scratch of the library's sorts, scans and merges: whoever needs more than there is grows it
static inline int ensure_sort_tmp(struct thj_ctx* c, size_t need) {
    return need > c->sort_tmp_bytes ? grow_device_buffer(c->d_sort_tmp, c->sort_tmp_bytes, need, need) : THJ_OK;
}
// the size query of a hipcub call, the scratch, the call: run(tmp, bytes) is the call with everything else bound
template <class Run>
static inline int run_with_sort_tmp(struct thj_ctx* c, Run run) {
    size_t need = 0;
    HIPCHK(run(nullptr, need));
    if (const int e = ensure_sort_tmp(c, need)) return e;
    size_t bytes = c->sort_tmp_bytes;
    HIPCHK(run(c->d_sort_tmp, bytes));
    return THJ_OK;
}
// one counter (or any small value) from the device, the stream idle behind it
template <class T>
static inline int read_device_value(struct thj_ctx* c, const T* d, T* h) {
    HIPCHK(hipMemcpyAsync(h, d, sizeof(T), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return THJ_OK;
}
// device temporaries of a call: freed on every way out (HIPCHK returns from the middle of a function).  hipFree waits for the device, so work
// still queued that reads them ends first.  A pointer handed to alloc() is declared before the DevTemps and handed over once
struct DevTemps {
    std::vector<void**> slots;
    DevTemps() = default; DevTemps(const DevTemps&) = delete;
    template <class T> hipError_t alloc(T*& p, size_t bytes) { p = nullptr; slots.push_back((void**)&p); return hipMalloc((void**)&p, bytes); }
    ~DevTemps() { for (void** p : slots) { (void)hipFree(*p); *p = nullptr; } }
};
hipEvent_t thj_get_event(struct thj_ctx* c);
int thj_ensure_aux_streams(struct thj_ctx* c, int need);            // thj_streams.hip: aux_stream[0 .. need)
void thj_warm_span(hipStream_t s); void thj_warm_ingest(hipStream_t s); void thj_warm_bamout(hipStream_t s);      // one empty launch from the translation unit: its code object is loaded now
int thj_dev_alloc(struct thj_ctx* c, void** out, size_t bytes);     // like hipMalloc, from the context's block cache
void thj_dev_release(struct thj_ctx* c, void* p);                  // like hipFree, but the block stays with the context
void thj_dev_cache_free(struct thj_ctx* c);
void thj_span_free(struct thj_ctx* c);
int thj_span_compact_device(struct thj_ctx* c, void** d_out);       // thj_span.hip: the pass's records, ordered, on the device
void thj_bamout_free(struct thj_ctx* c);                            // thj_bamout.hip
int thj_bam_stream_reserve(struct thj_ctx* c, size_t bytes);       // thj_bamout.hip: room for `bytes` in the context's BAM stream; its first bam_bytes bytes stay
// thj_ingest.hip, the front of thj_juncbed_add_bam: the records a piece of a BAM of reported alignments gives the consensus, in file
// order, on the device.  recs / ins_off live in the ingest arenas (until the context's next ingest call), ins_bases is the caller's to
// thj_dev_release; n_groups = the reads recs[].read_idx count over (fusions != 0); resume_*: where the next piece begins
// loc[i] / infl: where record i begins (its block_size field) in the inflated members, as member << 16 | offset -- infl + (member << 16) + offset
struct thj_reported_recs { thj_aln* recs; int64_t n; const int64_t* ins_off; uint8_t* ins_bases; int64_t n_groups; uint32_t resume_member, resume_skip;
                           const uint32_t* loc; const uint8_t* infl; };
int thj_ingest_reported(struct thj_ctx* c, const thj_bam_piece* piece, int32_t max_report_intron, int32_t indels, int32_t fusions, int32_t best, int32_t more_follows,
                        thj_reported_recs* out);

// thj_ingest.hip, the front of thj_juncbed_report_unmapped_bam: a piece of a reads file (unaligned BAM) inflated, every record located.  loc /
// infl as above (in the ingest arenas until the context's next ingest call); n_members: the piece's members, empty ones counted
struct thj_reads_recs { const uint32_t* loc; const uint8_t* infl; int64_t n; uint32_t n_members; };
int thj_ingest_reads_walk(struct thj_ctx* c, const thj_bam_piece* piece, thj_reads_recs* out);
// thj_unmapped.hip, for the add calls of thj_juncbed_impl.h while thj_juncbed_collect_unmapped is on.  thj_um_numbers_bam: before a piece's records
// are counted -- their reads' numbers from the QNAMEs, per record (THJ_EINVAL, nothing kept: not digits, 0, numbers that fall or repeat);
// thj_um_added: after an add call has counted its records -- n_units reads (or inserts) in all, numbered already (a piece) or waiting for
// thj_juncbed_read_numbers with these record counts per read (host arrays; runs == nullptr: inserts); has_l / has_r: how many have a group on that side
int thj_um_numbers_bam(struct thj_ctx* c, const thj_reported_recs* r);
void thj_um_added(struct thj_ctx* c, int64_t n_units, bool numbered, const uint32_t* runs, int64_t has_l, int64_t has_r);
int thj_um_add_ok(struct thj_ctx* c, const char* who);       // THJ_ESTATE: the call before still waits for its numbers

int thj_fusions_to_host(struct thj_ctx* c);        // h_fusions <- d_fus_out when it has not come down yet (thj_segjuncs.hip)
