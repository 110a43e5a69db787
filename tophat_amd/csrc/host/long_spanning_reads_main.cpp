// long_spanning_reads -- MI355X-native drop-in for TopHat's long_spanning_reads (same argv + files;
// tophat.py:3160-3191, parsed like long_spanning_reads.cpp:3151-3329).  Host C++ over include/thj.h.
// Contig segment maps (with any CIGAR, incl. N/I/D) and junction-db ("spliced") segment maps are supported, and so is
// --fusion-search: the .fusions list goes to the device, fused segment hits come from the fusion contigs of the junction
// database (BAM maps), fusion alignments leave as two records with XF:Z (print_bamhit / extract_partial_hits).
//
// The reads are cut into contiguous read-id shards with the reference's planner (calculate_offsets over the inputs' .index
// files, utils.cpp:22-127; long_spanning_reads.cpp:2983-3064).  Host workers ingest shards in parallel -- shard k's
// batches run on GPU k mod n -- and encode their records; with one output file a writer appends the shards' records in
// shard order (= read order), so the BAM stream and its .index do not depend on the number of shards; with -p N the N
// parts are the reference's N ranges, one file each (<base>{0..N-1}.bam).
#include <climits>
#include <deque>
#include <tuple>

#include "thj_bamrec.h"
#include "thj_driver.h"

using namespace thjh;

static std::atomic<long long> g_host_ingest_shards{0};      // shards the device-side ingest declined (the host readers took them)
static void print_usage() {
    fprintf(stderr, "Usage:   long_spanning_reads <reference.fasta> <reads.fq> <possible_juncs1,...,possible_juncsN> "
                    "<possible_insertions1,...,possible_insertionsN> <possible_deletions1,...,possible_deletionsN> "
                    "<possible_fusions1,...,possible_fusionsN> <out.bam> <seg1.bwtout,...,segN.bwtout> [spliced_seg1.bwtout,...,spliced_segN.bwtout]\n");
}

static PhaseTimer g_timer;
static WorkClock g_work;
// THJ_TRACE=1: one line per shard event on stderr (seconds since start): where a shard's time goes, for tools/lsr_trace.py
static const bool g_trace = getenv("THJ_TRACE") != nullptr;
static const long long g_trace_t0 = WorkClock::now();
static void trace(size_t shard, const char* what) { if (g_trace) fprintf(stderr, "[trace] %zu %s %.4f\n", shard, what, (double)(WorkClock::now() - g_trace_t0) * 1e-9); }

struct Shard {
    uint64_t begin_id = 0, end_id = ~0ull;
    int64_t read_off = 0, read_end = -1;            // read_end: where the next shard starts in the reads file (-1: the end)
    std::vector<int64_t> seg_off, spliced_off;
    std::vector<int64_t> seg_end;                   // where the next shard starts in the segment maps (-1: the end of the file)
    std::vector<int64_t> spliced_end;               // ... and in the junction-db maps
};

// long_spanning_reads.cpp:2983-2991, :3051-3064: index files in the order {reads, spliced maps last..first, contig maps
// last..first} -- the boundaries come from the FIRST segment's contig map, the stream the worker iterates over
static std::vector<Shard> plan(const std::string& reads, const std::vector<std::string>& segs, const std::vector<std::string>& spliced, int want) {
    std::vector<Shard> out(1);
    out[0].seg_off.assign(segs.size(), 0); out[0].spliced_off.assign(spliced.size(), 0); out[0].seg_end.assign(segs.size(), -1);
    out[0].spliced_end.assign(spliced.size(), -1);
    if (want < 2) return out;
    std::vector<std::string> fnames;
    fnames.push_back(reads);
    fnames.insert(fnames.end(), spliced.rbegin(), spliced.rend());
    fnames.insert(fnames.end(), segs.rbegin(), segs.rend());
    std::vector<IndexList> lists(fnames.size());
    size_t smallest = ~(size_t)0;
    for (size_t i = 0; i < fnames.size(); ++i) { load_index(fnames[i], want * 4, lists[i]); smallest = std::min(smallest, lists[i].size()); }
    if ((size_t)want > smallest) want = (int)smallest;
    std::vector<uint64_t> ids; std::vector<std::vector<int64_t>> offs;
    if (!calculate_offsets(lists, want, ids, offs)) return out;
    out.assign((size_t)want, Shard());
    for (int i = 0; i < want; ++i) {
        Shard& sh = out[(size_t)i];
        sh.seg_off.assign(segs.size(), 0); sh.spliced_off.assign(spliced.size(), 0);
        if (i > 0) {
            const std::vector<int64_t>& o = offs[(size_t)i - 1];
            sh.begin_id = ids[(size_t)i - 1];
            sh.read_off = o[0];
            for (size_t s = 0; s < spliced.size(); ++s) sh.spliced_off[s] = o[1 + (spliced.size() - 1 - s)];
            for (size_t s = 0; s < segs.size(); ++s) sh.seg_off[s] = o[1 + spliced.size() + (segs.size() - 1 - s)];
        }
        sh.end_id = i + 1 < want ? ids[(size_t)i] : ~0ull;
    }
    for (int i = 0; i < want; ++i) {
        Shard& sh = out[(size_t)i];
        sh.seg_end.assign(segs.size(), -1);
        sh.spliced_end.assign(spliced.size(), -1);
        // lists = {reads, spliced maps last..first, contig maps last..first}
        if (i + 1 < want) for (size_t s = 0; s < segs.size(); ++s) sh.seg_end[s] = shard_end_offset(lists[1 + spliced.size() + (segs.size() - 1 - s)], sh.end_id);
        if (i + 1 < want) for (size_t s = 0; s < spliced.size(); ++s) sh.spliced_end[s] = shard_end_offset(lists[1 + (spliced.size() - 1 - s)], sh.end_id);
        if (i + 1 < want) sh.read_end = shard_end_offset(lists[0], sh.end_id);
    }
    return out;
}

// ------------------------------------------------------------------ the junction / indel / fusion lists
// every line (without its newline) of every file of a comma-separated list; a file that does not open is skipped
template <class F>
static void for_each_line(const std::string& list, bool warn_missing, F on_line) {
    for (auto& fn : split(list, ',')) {
        FILE* f = fopen(fn.c_str(), "r");
        if (!f) { if (warn_missing) fprintf(stderr, "Warning: cannot open %s\n", fn.c_str()); continue; }
        char buf[2048];
        while (fgets(buf, sizeof buf, f)) {
            char* nl = strrchr(buf, '\n'); if (nl) *nl = 0;
            on_line(buf);
        }
        fclose(f);
    }
}
template <class T, class Less>
static void sort_unique(std::vector<T>& v, Less less) {
    std::sort(v.begin(), v.end(), less);
    v.erase(std::unique(v.begin(), v.end(), [&](const T& a, const T& b) { return !less(a, b) && !less(b, a); }), v.end());
}

// junctions + deletions -> std::set<Junction> (long_spanning_reads.cpp:2897-2944)
static std::vector<thj_junction> load_junctions(RefTable& rt, const std::string& junc_list, const std::string& del_list) {
    std::vector<thj_junction> juncs;
    for_each_line(junc_list, true, [&](const char* buf) {                       // a missing file warns (:3245-3251)
        char name[256]; int l, r; char ori;
        if (sscanf(buf, "%255s %d %d %c", name, &l, &r, &ori) != 4) return;
        juncs.push_back({rt.get_id(name), (uint32_t)l, (uint32_t)r, ori == '-' ? 1u : 0u});
    });
    for_each_line(del_list, false, [&](const char* buf) {
        std::vector<std::string> t = split(buf, '\t');
        if (t.size() < 3) die("Error: malformed deletion coordinate record\n");
        juncs.push_back({rt.get_id(t[0]), (uint32_t)atoi(t[1].c_str()) - 1u, (uint32_t)atoi(t[2].c_str()), 0u});
    });
    sort_unique(juncs, [](const thj_junction& a, const thj_junction& b) {        // junctions.h:39-57
        return std::tie(a.ref_id, a.left, a.right, a.antisense) < std::tie(b.ref_id, b.left, b.right, b.antisense);
    });
    return juncs;
}

// insertions -> std::set<Insertion>: first inserted wins among equal (ref,left,len) (:2952-2980, insertions.h:52-67);
// four words per entry: ref, left, length, the bases at three bits each
static std::vector<uint32_t> load_insertions(RefTable& rt, const std::string& list) {
    struct InsRow { uint32_t ref, left, len, seq; size_t order; };
    std::vector<InsRow> ins;
    for_each_line(list, false, [&](const char* buf) {
        std::vector<std::string> t = split(buf, '\t');
        if (t.size() < 4) die("Error: malformed insertion coordinate record\n");
        uint32_t code = 0;
        if (t[3].size() > 6) die("Error: insertion longer than 6 bases is not supported by this build\n");
        for (size_t k = 0; k < t[3].size(); ++k) {
            uint32_t c = 4;
            switch (t[3][k]) { case 'A': case 'a': c = 0; break; case 'C': case 'c': c = 1; break; case 'G': case 'g': c = 2; break; case 'T': case 't': c = 3; break; }
            code |= c << (3 * k);
        }
        ins.push_back({rt.get_id(t[0]), (uint32_t)atoi(t[1].c_str()), (uint32_t)t[3].size(), code, ins.size()});
    });
    std::stable_sort(ins.begin(), ins.end(), [](const InsRow& a, const InsRow& b) { return std::tie(a.ref, a.left, a.len) < std::tie(b.ref, b.left, b.len); });
    std::vector<uint32_t> ins_tab;
    for (size_t i = 0; i < ins.size(); ++i) {
        if (i && ins[i].ref == ins[i - 1].ref && ins[i].left == ins[i - 1].left && ins[i].len == ins[i - 1].len) continue;
        ins_tab.insert(ins_tab.end(), {ins[i].ref, ins[i].left, ins[i].len, ins[i].seq});
    }
    return ins_tab;
}

// --fusion-search: the .fusions lists -> std::set<Fusion> (:2998-3040, fusions.h:44-71)
static std::vector<thj_span_fusion> load_fusions(RefTable& rt, const std::string& list) {
    std::vector<thj_span_fusion> fusions;
    for_each_line(list, false, [&](const char* buf) {
        std::vector<std::string> t;                      // strsep: empty fields count
        { const char* b0 = buf; for (const char* q = buf;; ++q) if (*q == '\t' || !*q) { t.emplace_back(b0, q); if (!*q) break; b0 = q + 1; } }
        if (t.size() < 5) die("Error: malformed insertion coordinate record\n");
        uint32_t dir = THJ_CIG_FUSION_FF;
        if (t[4] == "fr") dir = THJ_CIG_FUSION_FR; else if (t[4] == "rf") dir = THJ_CIG_FUSION_RF; else if (t[4] == "rr") dir = THJ_CIG_FUSION_RR;
        fusions.push_back({rt.get_id(t[0]), rt.get_id(t[2]), (uint32_t)atoi(t[1].c_str()), (uint32_t)atoi(t[3].c_str()), dir});
    });
    sort_unique(fusions, [](const thj_span_fusion& a, const thj_span_fusion& b) {
        return std::tie(a.ref_id1, a.ref_id2, a.left, a.right, a.dir) < std::tie(b.ref_id1, b.ref_id2, b.left, b.right, b.dir);
    });
    return fusions;
}

// the sets the stitch kernels close gaps with: sorted, without duplicates
struct SpanSets {
    std::vector<thj_junction> juncs;
    std::vector<uint32_t> ins_tab;
    std::vector<thj_span_fusion> fusions;
};
// pos[2..5]: the junction, insertion, deletion and fusion lists of the command line, in the order the reference reads them
static SpanSets load_span_sets(RefTable& rt, const std::vector<std::string>& pos, bool fusion_search) {
    SpanSets s;
    s.juncs = load_junctions(rt, pos[2], pos[4]);
    s.ins_tab = load_insertions(rt, pos[3]);
    if (fusion_search) s.fusions = load_fusions(rt, pos[5]);
    return s;
}

// ------------------------------------------------------------------ shards and threads
static int64_t input_bytes(const std::string& reads, const std::vector<std::string>& segs) {
    int64_t n = 0;
    struct stat sb;
    for (const std::string& f : segs) if (!stat(f.c_str(), &sb)) n += (int64_t)sb.st_size;
    if (!stat(reads.c_str(), &sb)) n += (int64_t)sb.st_size;
    return n;
}
static int env_int(const char* name, int fallback, int at_least = INT_MIN) { return getenv(name) && atoi(getenv(name)) >= at_least ? atoi(getenv(name)) : fallback; }

struct RunPlan {
    int hw = 1, workers = 1;
    int parts = 1;                                  // output files (-p N: the reference's N ranges, one file each)
    std::vector<Shard> shards;
    size_t lookahead = 32;                          // shards in flight (memory bound)
    size_t batch_reads = (size_t)1 << 19;
    int enc_threads = 1;
    int feeders = 1, pool_threads = 2;
};
// -p N: the reference's N ranges, one output file each.  One output file: our own number of shards, written in order.
static RunPlan plan_run(const Opts& o, const std::string& reads, const std::vector<std::string>& segs, const std::vector<std::string>& spliced,
                        int64_t in_bytes, bool dev_ingest, int n_gpus) {
    RunPlan r;
    r.hw = effective_cpus();
    r.workers = std::max(1, env_int("THJ_WORKERS", std::max(1, std::min(32, r.hw * 3 / 4))));
    r.parts = o.num_threads > 1 ? o.num_threads : 1;
    if (r.parts > 1) {
        r.shards = plan(reads, segs, spliced, r.parts);
        if ((int)r.shards.size() != r.parts) r.parts = 1;         // not enough data: one thread (:2992-2993)
    }
    if (r.parts == 1) {
        // shards of ~16 MB of compressed input (~110 k reads of 100 bases with four segment maps): measured best for the pipeline below
        // (10 M pairs: 24 MB 1.02-1.15 s per side, 16 MB 0.83-0.93, 12 MB 0.80-0.92, 8 MB 0.96-1.11, 48 MB 1.49) -- and at least four per host worker
        const uint64_t shard_mb = (uint64_t)env_int("THJ_SHARD_MB", 16, 1);
        int n_shards = getenv("THJ_SHARD_MB") ? 1 : 4 * r.workers;
        const uint64_t by_size = (uint64_t)in_bytes / (shard_mb << 20);
        if (getenv("THJ_SHARDS")) n_shards = atoi(getenv("THJ_SHARDS"));
        else if (by_size > (uint64_t)n_shards) n_shards = (int)std::min<uint64_t>(by_size, 4096);
        r.shards = plan(reads, segs, spliced, n_shards);
    }
    const size_t S = r.shards.size();
    r.lookahead = getenv("THJ_LOOKAHEAD") ? (size_t)atoll(getenv("THJ_LOOKAHEAD")) : (size_t)std::max(r.workers + 2, 32);
    if (getenv("THJ_BATCH_READS")) r.batch_reads = (size_t)atoll(getenv("THJ_BATCH_READS"));
    r.enc_threads = S == 1 ? host_threads() : 1;    // many shards: the workers are the parallelism
    // thread counts: with the device-side ingest a feeder mostly waits for the GPU (a few per context keep it fed) and the pool has the
    // CPUs; with the host readers the feeders parse, so they are the old workers and the pool gets what is left
    const bool split_roles = dev_ingest && r.parts == 1;
    r.feeders = env_int("THJ_FEEDERS", split_roles ? 2 * n_gpus + 2 : r.workers, 1);
    r.pool_threads = env_int("THJ_POOL", split_roles ? std::max(2, r.hw - 2) : std::max(2, r.hw - r.workers), 1);
    return r;
}

// ------------------------------------------------------------------ the pipeline's threads
// The run is a pipeline of three kinds of threads (one output file; with -p N every part writes its own file from its feeder):
//   feeders   a few per GPU context: a shard's device work (ingest, stitch, download), shard after shard -- they wait on the
//             GPU, not on the CPU;
//   the pool  record encoding and BGZF deflate as independent jobs: the CPU-heavy part, never waiting for anything;
//   writer    the main thread: appends the deflated members in shard order, computes `.index` lines.
// Where BGZF members end depends on the bytes still open from the shard before, so shards are PLANNED in output order -- cheap,
// record sizes only, done by whichever thread delivers the shard that was missing (Planner::deliver) -- and DEFLATED
// independently afterwards (BamWriter::plan / compress / commit).  Before this split every worker did all of it for its shard
// and the run moved in waves: all workers on the GPU's lock, then all deflating while the GPU idled (THJ_TRACE, tools/lsr_trace.py).
struct Pool {
    std::mutex mu; std::condition_variable cv; std::deque<std::function<void()>> q; bool stop = false; std::vector<std::thread> th;
    void start(int n) { for (int t = 0; t < n; ++t) th.emplace_back([this] { run(); }); }
    void run() {
        for (;;) {
            std::function<void()> f;
            { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return stop || !q.empty(); }); if (q.empty()) return; f = std::move(q.front()); q.pop_front(); }
            f();
        }
    }
    void submit(std::function<void()> f) { { std::lock_guard<std::mutex> lk(mu); q.push_back(std::move(f)); } cv.notify_one(); }
    void finish() { { std::lock_guard<std::mutex> lk(mu); stop = true; } cv.notify_all(); for (auto& t : th) t.join(); th.clear(); }
};

// records of one shard on their way to the writer
struct OutShard {
    std::mutex mu; std::condition_variable cv;
    std::deque<BamWriter::Prepared> q;
    bool done = false;
};

// One output file: the shards' records in shard order.  deliver() takes a shard's records -- all of them: one call per shard, an
// empty one for a shard without records -- and plans every shard that is now next in line; write_in_order() is the writer.
struct Planner {
    struct Slot { BamWriter::Encoded e; bool ready = false; BamWriter::Prepared p; };
    Pool& pool;
    std::vector<Slot> so;
    std::vector<std::unique_ptr<OutShard>> outq;
    std::mutex plan_mu;
    size_t plan_next = 0;                                      // the first shard not planned yet
    std::vector<uint8_t> plan_carry;                           // bytes of the open block after the last planned shard
    std::mutex win_mu; std::condition_variable win_cv;
    size_t writer_pos = 0;                                     // shards before this one are on disk
    size_t lookahead;

    Planner(Pool& pool_, size_t n_shards, size_t lookahead_) : pool(pool_), so(n_shards), lookahead(lookahead_) {
        for (size_t k = 0; k < n_shards; ++k) outq.emplace_back(new OutShard());
    }
    // a feeder starts shard k only when the writer is at most `lookahead` shards behind
    void wait_for_turn(size_t k) { std::unique_lock<std::mutex> lk(win_mu); win_cv.wait(lk, [&] { return k < writer_pos + lookahead; }); }
    void deflate_shard(size_t j) {
        BamWriter::compress(so[j].p);
        trace(j, "deflated");
        OutShard& oq = *outq[j];
        std::lock_guard<std::mutex> lk(oq.mu);
        oq.q.push_back(std::move(so[j].p));
        oq.done = true;
        oq.cv.notify_all();
    }
    // records encoded on the host, or -- encoded and deflated on the device -- a Prepared that only needs what the shard before
    // left open closed
    static void put(Slot& s, BamWriter::Encoded&& e) { s.e = std::move(e); }
    static void put(Slot& s, BamWriter::Prepared&& dp) { s.p = std::move(dp); }
    template <class Records>
    void deliver(size_t k, Records&& rec) {
        std::vector<size_t> planned;
        {
            std::lock_guard<std::mutex> lk(plan_mu);
            put(so[k], std::move(rec)); so[k].ready = true;
            for (; plan_next < so.size() && so[plan_next].ready; ++plan_next) {
                Slot& s = so[plan_next];
                if (s.p.device) BamWriter::plan_device(plan_carry, s.p);
                else BamWriter::plan(plan_carry, std::move(s.e), s.p);
                trace(plan_next, "planned");
                planned.push_back(plan_next);
            }
        }
        for (size_t i = 1; i < planned.size(); ++i) pool.submit([this, j = planned[i]] { deflate_shard(j); });
        if (!planned.empty()) deflate_shard(planned[0]);
    }
    // the next batch of shard k, false when the shard is through
    bool next_prepared(size_t k, BamWriter::Prepared& e) {
        OutShard& oq = *outq[k];
        std::unique_lock<std::mutex> lk(oq.mu);
        oq.cv.wait(lk, [&] { return !oq.q.empty() || oq.done; });
        if (oq.q.empty()) return false;
        e = std::move(oq.q.front());
        oq.q.pop_front();
        oq.cv.notify_all();
        return true;
    }
    // the writer: shard after shard, batch after batch -- the members arrive deflated, this thread appends them
    void write_in_order(BamWriter& bw) {
        for (size_t k = 0; k < so.size(); ++k) {
            for (BamWriter::Prepared e; next_prepared(k, e); e = BamWriter::Prepared()) {
                bw.commit(e);
                trace(k, "written");
            }
            { std::lock_guard<std::mutex> lk(win_mu); writer_pos = k + 1; }
            win_cv.notify_all();
        }
    }
};

// ------------------------------------------------------------------ the run
// what every shard of the run shares
struct Run {
    Opts& o;
    RefTable& rt;
    const std::string& reads_fn;
    const std::vector<std::string>& segs;
    const std::vector<std::string>& spliced_segs;
    const SpanSets& sets;
    const RunPlan& plan;
    std::vector<std::unique_ptr<Gpu>>& gpus;
    // BAM segment maps mapped for the device-side ingest, and the reads file when it is an (unaligned) BAM
    std::vector<std::unique_ptr<BamFile>>& bams;
    // ... the junction-db maps the same way, and the target table of their common header (thj_juncdb_target, once per context)
    std::vector<std::unique_ptr<BamFile>>& sbams;
    const std::vector<thj_juncdb_target>& juncdb;
    BamFile& reads_bam;
    bool dev_ingest, dev_reads, dev_out;            // on the device: the maps' ingest, the reads' too, the output records
    std::vector<std::unique_ptr<BamWriter>>& bws;   // one, or one per part
    Pool& pool;
    Planner& planner;
    std::vector<int32_t> tid_of_ref;                // dev_out: the output header's target of every contig
    std::atomic<long long> dev_out_shards{0}, host_out_shards{0};

    int nseg() const { return (int)segs.size(); }
    // HIP start-up (0.15-0.25 s) runs beside the first shards' ingest: a GPU's context is picked up -- with the genome and
    // the sets going up then -- the first time a worker needs that device (under the GPU's lock).
    thj_ctx* device_ready(Gpu& g) {
        if (g.ctx) return g.ctx;
        g.ctx = g.fut.get();
        rt.upload(g.ctx);
        if (thj_span_sets_upload(g.ctx, sets.juncs.data(), (int64_t)sets.juncs.size(), sets.ins_tab.data(), (int64_t)sets.ins_tab.size() / 4)) die("Error: %s\n", thj_last_error());
        if (o.fusion_search && thj_span_fusions_upload(g.ctx, sets.fusions.data(), (int64_t)sets.fusions.size())) die("Error: %s\n", thj_last_error());
        // (fusion contigs of the junction database are spliced on the device as well: the switch belongs to the table just uploaded)
        if (dev_ingest && !juncdb.empty() && (thj_span_juncdb_upload(g.ctx, juncdb.data(), (int64_t)juncdb.size()) || thj_span_juncdb_fusion_contigs(g.ctx, 1)))
            die("Error: %s\n", thj_last_error());
        if (dev_out) {                               // XF:Z of a fusion alignment names both contigs
            std::vector<const char*> names;
            for (const std::string& name : rt.names) names.push_back(name.c_str());
            if (thj_bam_contig_names_upload(g.ctx, names.data(), (int32_t)names.size())) die("Error: %s\n", thj_last_error());
        }
        if (thj_span_reset_async(g.ctx)) die("Error: %s\n", thj_last_error());
        return g.ctx;
    }
};

// reads on their way to the device: text back to back, where each read ends, the longest
struct ReadText {
    std::vector<int64_t> off{0};
    std::string bases, quals;
    size_t max_len = 0;
    void add(const Read& rd) {
        bases += rd.seq; quals += rd.qual;
        off.push_back((int64_t)bases.size());
        if (rd.seq.size() > max_len) max_len = rd.seq.size();
    }
    void clear() { off.assign(1, 0); bases.clear(); quals.clear(); max_len = 0; }
    int64_t n() const { return (int64_t)off.size() - 1; }
};

// The stitch pass over a batch on the device; returns the number of alignments.  THJ_ERETRY: a device pool was enlarged, the
// pass runs again.
static int64_t stitch(size_t k, thj_ctx* ctx, const thj_params& p, thj_span_batch* dev) {
    int64_t na = 0;
    for (int attempt = 0;; ++attempt) {
        if (thj_span_reset_async(ctx)) die("Error: %s\n", thj_last_error());
        if (thj_span_run_async(ctx, &p, dev)) die("Error: %s\n", thj_last_error());
        const int frc = thj_span_finish(ctx, &na);
        if (frc == THJ_ERETRY && attempt < 4) { trace(k, "stitch_retry"); continue; }
        if (frc) die("Error: %s\n", thj_last_error());
        return na;
    }
}

// ---- a shard whose maps the device took in (thj_ingest_span_hits / thj_ingest_span_batch)
// what the ingest hands back; owns its host buffers until a step takes them over
struct Ingested {
    int rc = THJ_OK;
    thj_span_batch* dev = nullptr;                  // the batch on the device (freed under the GPU's lock, thj_span_batch_free); null: no reads
    int64_t n = 0;
    uint32_t* ids = nullptr;                        // the rows' read ids
    uint8_t* rinfl = nullptr; int64_t rinfl_bytes = 0;        // the inflated read records (page-locked) and ...
    uint32_t* rloc = nullptr;                       // ... where each row's record lies in them: where the host encodes the records
    ~Ingested() { free(ids); free(rloc); thj_pinned_free(rinfl); }
};

// what the host encoder needs of a shard once its device work is done: the rows' reads, the records they point into, the alignments
struct HostRecords {
    std::vector<Read> reads;
    uint8_t* rinfl = nullptr;
    std::vector<thj_aln> alns;                      // -p N
    thj_aln* alns_pinned = nullptr; int64_t n_alns = 0;       // one output file: the records come down into a page-locked buffer
    void release() { thj_pinned_free(rinfl); thj_pinned_free(alns_pinned); rinfl = nullptr; alns_pinned = nullptr; std::vector<Read>().swap(reads); std::vector<thj_aln>().swap(alns); }
    ~HostRecords() { release(); }
    // the rows' own BAM records, where the host encoder copies names, bases and qualities from
    void rows_from_raw(Ingested& in) {
        for (int64_t r = 0; r < in.n; ++r) {
            const uint32_t loc = in.rloc[r];
            reads[(size_t)r].raw = in.rinfl + ((size_t)(loc >> 16) << 16) + (loc & 0xFFFFu) + 4;
        }
        free(in.rloc); in.rloc = nullptr;
        rinfl = in.rinfl; in.rinfl = nullptr;
    }
};

static void ingest_on_device(Run& R, size_t k, Gpu& gpu, Ingested& in) {
    const Shard& sh = R.plan.shards[k];
    const int nseg = R.nseg();
    std::vector<thj_bam_piece> segp;
    for (int s = 0; s < nseg; ++s) segp.push_back(R.bams[(size_t)s]->piece(sh.seg_off[(size_t)s], sh.seg_end.empty() ? -1 : sh.seg_end[(size_t)s]));
    const int nspl = (int)R.sbams.size();              // junction-db map s belongs to segment s
    std::vector<thj_bam_piece> splp;
    for (int s = 0; s < nspl; ++s) {
        splp.push_back(R.sbams[(size_t)s]->piece(sh.spliced_off[(size_t)s], sh.spliced_end.empty() ? -1 : sh.spliced_end[(size_t)s]));
        splp.back().n_tid = 0; splp.back().tid2ref = nullptr;       // its targets are the context's table (device_ready), not a list per shard
    }
    thj_bam_piece rp = R.dev_reads ? R.reads_bam.piece(sh.read_off, sh.read_end) : thj_bam_piece{};
    const uint32_t b_id = clamp_id32(sh.begin_id), e_id = clamp_id32(sh.end_id);
    // the shard's compressed pieces go into one page-locked buffer first -- here, beside the other feeders and outside the GPU's
    // lock: from the mapped files the copy up runs through the runtime's staging buffers at ~3 GB/s while the pool keeps the
    // CPUs busy, from page-locked memory it is DMA
    std::vector<std::pair<const BamFile*, thj_bam_piece*>> to_stage;
    for (int s = 0; s < nseg; ++s) to_stage.emplace_back(R.bams[(size_t)s].get(), &segp[(size_t)s]);
    for (int s = 0; s < nspl; ++s) to_stage.emplace_back(R.sbams[(size_t)s].get(), &splp[(size_t)s]);
    if (R.dev_reads) to_stage.emplace_back(&R.reads_bam, &rp);
    uint8_t* stage = stage_pieces(to_stage);
    {
        GpuLock lk(gpu, g_work);
        trace(k, "ingest_begin");
        thj_ctx* ctx = R.device_ready(gpu);
        const bool host_copy = R.dev_reads && !R.dev_out;       // the host encoder needs the rows' own records
        if (nspl) in.rc = thj_ingest_span_batch_spliced(ctx, &R.o.p, nseg, segp.data(), nspl, splp.data(), R.dev_reads ? &rp : nullptr, b_id, e_id, &in.dev, &in.ids, &in.n,
                                                        host_copy ? &in.rinfl : nullptr, host_copy ? &in.rinfl_bytes : nullptr, host_copy ? &in.rloc : nullptr);
        else if (R.dev_reads && R.dev_out) in.rc = thj_ingest_span_batch(ctx, &R.o.p, nseg, segp.data(), &rp, b_id, e_id, &in.dev, &in.ids, &in.n, nullptr, nullptr, nullptr);
        else if (R.dev_reads) in.rc = thj_ingest_span_batch(ctx, &R.o.p, nseg, segp.data(), &rp, b_id, e_id, &in.dev, &in.ids, &in.n, &in.rinfl, &in.rinfl_bytes, &in.rloc);
        else in.rc = thj_ingest_span_hits(ctx, &R.o.p, nseg, segp.data(), b_id, e_id, &in.dev, &in.ids, &in.n);
        trace(k, "ingest_end");
    }
    thj_pinned_free(stage);
}

// the reads of the batch's rows: the rows' own BAM records when the device inflated the reads file (they are attached to the batch
// already), else fetched by id from the ReadStream and packed for the device
static PackedReads reads_for_batch(Run& R, size_t k, Ingested& in, HostRecords& hr) {
    hr.reads.resize((size_t)in.n);
    PackedReads packed;
    if (R.dev_reads) {
        for (int64_t r = 0; r < in.n; ++r) hr.reads[(size_t)r].id = in.ids[r];
        if (!R.dev_out) hr.rows_from_raw(in);
    } else {
        ReadStream reads;
        if (!reads.open(R.reads_fn, R.o.zpacker, R.plan.shards[k].read_off)) die("Error: cannot open %s for reading\n", R.reads_fn.c_str());
        ReadText text;
        for (int64_t r = 0; r < in.n; ++r) {
            if (!reads.get(in.ids[r], hr.reads[(size_t)r])) die("Error: could not get read # %d from stream\n", (int)in.ids[r]);
            text.add(hr.reads[(size_t)r]);
        }
        packed = pack_reads(text.off, text.bases, text.max_len, &text.quals);
    }
    free(in.ids); in.ids = nullptr;
    return packed;
}

// a shard's records as the device made them: record sizes, read ids, and the deflated members back to back in a page-locked buffer
struct DeviceMembers {
    std::vector<uint32_t> size; std::vector<int64_t> rid;
    std::vector<size_t> cuts; std::vector<uint32_t> clen, crc;
    uint8_t* comp = nullptr; int64_t comp_bytes = 0;
    ~DeviceMembers() { thj_pinned_free(comp); }
};
// Records and BGZF members on the device (under the GPU's lock); the host gets record sizes, read ids and the deflated members.
// false: the device declined the shard (THJ_EFALLBACK) -- the rows' reads come back instead, for the host encoder.
static bool records_on_device(Run& R, size_t k, thj_ctx* ctx, Ingested& in, int64_t na, DeviceMembers& m, HostRecords& hr) {
    m.size.resize(2 * (size_t)na); m.rid.resize(2 * (size_t)na);       // a fusion alignment is two records
    int64_t total = 0, n_rec = 0;
    int erc = thj_span_bam_encode_records(ctx, in.dev, R.tid_of_ref.data(), (int32_t)R.tid_of_ref.size(), 2 * na, m.size.data(), m.rid.data(), &n_rec, &total);
    if (erc == THJ_OK) {
        m.size.resize((size_t)n_rec); m.rid.resize((size_t)n_rec);
        trace(k, "bam_encoded");
        BamWriter::plan_cuts_closed(m.size, m.cuts);
        std::vector<int64_t> ends(m.cuts.begin(), m.cuts.end());
        m.clen.resize(m.cuts.size()); m.crc.resize(m.cuts.size());
        m.comp = (uint8_t*)thj_pinned_alloc(m.cuts.size() * (size_t)65536 + 64);
        if (!m.comp) die("Error: out of memory\n");
        erc = thj_bgzf_deflate(ctx, (int64_t)m.cuts.size(), ends.data(), m.comp, (int64_t)(m.cuts.size() * (size_t)65536), m.clen.data(), m.crc.data(), &m.comp_bytes);
        trace(k, "bam_deflated");
    }
    if (erc == THJ_OK) return true;
    if (erc != THJ_EFALLBACK) die("Error: %s\n", thj_last_error());
    static std::atomic<bool> told{false};
    if (!told.exchange(true)) fprintf(stderr, "\tdevice-side BAM output not possible for a shard (%s); encoding on the host\n", thj_last_error());
    thj_pinned_free(m.comp); m.comp = nullptr;
    if (thj_span_batch_reads_host(ctx, in.dev, &in.rinfl, &in.rinfl_bytes, &in.rloc)) die("Error: %s\n", thj_last_error());
    hr.rows_from_raw(in);
    return false;
}
// outside the GPU's lock: the members into their BGZF envelopes
static BamWriter::Prepared wrap_members(DeviceMembers& m) {
    BamWriter::Prepared dp;
    dp.device = true;
    dp.size = std::move(m.size);
    dp.rid.assign(m.rid.begin(), m.rid.end());
    dp.cuts = std::move(m.cuts);
    dp.members.resize(dp.cuts.size());
    size_t at = 0;
    for (size_t i = 0; i < dp.cuts.size(); ++i) {
        const size_t ulen = dp.cuts[i] - (i ? dp.cuts[i - 1] : 0);
        BamWriter::wrap_member(m.comp + at, m.clen[i], m.crc[i], (uint32_t)ulen, dp.members[i]);
        at += m.clen[i];
    }
    if ((int64_t)at != m.comp_bytes) die("Error: the device deflater's member sizes do not add up\n");
    thj_pinned_free(m.comp); m.comp = nullptr;
    return dp;
}

// the alignments down to the host (under the GPU's lock)
static void download_alns(Run& R, size_t k, thj_ctx* ctx, int64_t na, HostRecords& hr) {
    hr.n_alns = na;
    if (R.plan.parts > 1) hr.alns.resize((size_t)na);
    else if (!(hr.alns_pinned = (thj_aln*)thj_pinned_alloc((size_t)(na ? na : 1) * sizeof(thj_aln)))) die("Error: out of memory\n");
    trace(k, "stitch_resized");
    if (na && thj_span_download(ctx, R.plan.parts > 1 ? hr.alns.data() : hr.alns_pinned)) die("Error: %s\n", thj_last_error());
    trace(k, "stitch_downloaded");
}

// Records on the host.  -p N: encoded here and written to the part's own file.  One output file: the CPU part of the shard goes
// to the pool; this feeder moves on to the next shard's device work.
static void records_on_host(Run& R, size_t k, std::shared_ptr<HostRecords> hr) {
    if (R.plan.parts > 1) {
        BamWriter::Encoded e;
        const long long te = WorkClock::now();
        encode_batch(*R.bws[k], R.rt, hr->alns.data(), hr->alns.size(), hr->reads, R.plan.enc_threads, e);
        g_work.add(3, te);
        hr->release();
        R.bws[k]->write_encoded(e);
        return;
    }
    R.pool.submit([&R, k, hr] {
        BamWriter::Encoded e;
        const long long te = WorkClock::now();
        encode_batch(*R.bws[0], R.rt, hr->alns_pinned, (size_t)hr->n_alns, hr->reads, 1, e);
        g_work.add(3, te);
        trace(k, "encoded");
        hr->release();
        R.planner.deliver(k, std::move(e));
    });
}

// the rest of a shard after its ingest on the device: reads, stitch, records
static void finish_ingested_shard(Run& R, size_t k, Gpu& gpu, Ingested& in) {
    auto hr = std::make_shared<HostRecords>();
    const PackedReads packed = reads_for_batch(R, k, in, *hr);
    DeviceMembers members;
    bool on_device = false;                          // the shard's records were encoded and deflated on the device
    {
        GpuLock lk(gpu, g_work);
        trace(k, "stitch_begin");
        thj_ctx* ctx = R.device_ready(gpu);
        if (!R.dev_reads && thj_span_batch_attach_reads(ctx, in.dev, packed.W, packed.stride, packed.planes.data(), packed.lens.data(), packed.quals.data())) die("Error: %s\n", thj_last_error());
        const int64_t na = stitch(k, ctx, R.o.p, in.dev);
        trace(k, "stitch_finished");
        if (R.dev_out) on_device = records_on_device(R, k, ctx, in, na, members, *hr);
        if (!on_device) download_alns(R, k, ctx, na, *hr);
        if (thj_span_batch_free(ctx, in.dev)) die("Error: %s\n", thj_last_error());
        in.dev = nullptr;
        trace(k, "stitch_end");
    }
    if (on_device) {
        ++R.dev_out_shards;
        BamWriter::Prepared dp = wrap_members(members);
        trace(k, "wrapped");
        R.planner.deliver(k, std::move(dp));
        return;
    }
    ++R.host_out_shards;
    records_on_host(R, k, std::move(hr));
}

// ---- a shard through the host readers
// one batch of the host readers' merge: the rows' reads, their segment hit lists, the reads' text
struct HostBatch {
    std::vector<Read> reads;
    std::vector<uint32_t> seg_off{0};
    std::vector<thj_span_hit> hits;
    ReadText text;
    void clear() { reads.clear(); seg_off.assign(1, 0); hits.clear(); text.clear(); }
};

// upload, stitch, download, encode; with one output file the shard's batches gather in shard_e (the planner takes whole shards)
static void flush_host_batch(Run& R, size_t k, Gpu& gpu, HostBatch& b, BamWriter::Encoded& shard_e) {
    const int64_t n = b.text.n();
    if (n == 0) return;
    const PackedReads packed = pack_reads(b.text.off, b.text.bases, b.text.max_len, &b.text.quals);
    thj_span_batch hb{};
    hb.n_reads = (int32_t)n; hb.nseg = R.nseg(); hb.words_per_plane = packed.W; hb.qual_stride = packed.stride;
    hb.seg_off = b.seg_off.data(); hb.hits = b.hits.data(); hb.read_planes = packed.planes.data(); hb.read_len = packed.lens.data(); hb.quals = packed.quals.data();
    std::vector<thj_aln> alns;
    {
        GpuLock lk(gpu, g_work);
        thj_ctx* ctx = R.device_ready(gpu);
        thj_span_batch* dev = nullptr;
        if (thj_span_batch_upload(ctx, &hb, (int64_t)b.hits.size(), &dev)) die("Error: %s\n", thj_last_error());
        const int64_t na = stitch(k, ctx, R.o.p, dev);
        alns.resize((size_t)na);
        if (na && thj_span_download(ctx, alns.data())) die("Error: %s\n", thj_last_error());
        if (thj_span_batch_free(ctx, dev)) die("Error: %s\n", thj_last_error());
    }
    BamWriter::Encoded e;
    const long long te = WorkClock::now();
    encode_batch(*R.bws[R.plan.parts == 1 ? 0 : k], R.rt, alns.data(), alns.size(), b.reads, R.plan.enc_threads, e);
    g_work.add(3, te);
    if (R.plan.parts > 1) R.bws[k]->write_encoded(e);         // this part's own file
    else {
        shard_e.bytes.insert(shard_e.bytes.end(), e.bytes.begin(), e.bytes.end());
        shard_e.size.insert(shard_e.size.end(), e.size.begin(), e.size.end());
        shard_e.rid.insert(shard_e.rid.end(), e.rid.begin(), e.rid.end());
    }
    b.clear();
}

// the stream's group of read `id`, if it has one, appended to g; groups of smaller ids are passed over
static void take_group(HitStream& hs, uint32_t id, std::vector<Hit>& g) {
    while (hs.next_group_id() && hs.next_group_id() < id) hs.skip_group();
    if (hs.next_group_id() == id) hs.next_group(g);
}

static void run_shard_host_readers(Run& R, size_t k, Gpu& gpu) {
    const Shard& sh = R.plan.shards[k];
    const int nseg = R.nseg();
    std::vector<HitStream> st((size_t)nseg);
    for (int s = 0; s < nseg; ++s)
        if (!st[(size_t)s].open(R.segs[(size_t)s], R.rt, R.o.p, false, sh.seg_off[(size_t)s], sh.begin_id, sh.end_id))
            die("Error opening SAM file %s\n", R.segs[(size_t)s].c_str());
    // junction-db ("spliced") segment maps: SplicedBAMHitFactory streams, one per segment (:3110-3123)
    std::vector<HitStream> sst(R.spliced_segs.size());
    for (size_t s = 0; s < sst.size(); ++s)
        if (!sst[s].open(R.spliced_segs[s], R.rt, R.o.p, true, sh.spliced_off[s], sh.begin_id, sh.end_id)) die("Error opening SAM file %s\n", R.spliced_segs[s].c_str());
    ReadStream reads;
    if (!reads.open(R.reads_fn, R.o.zpacker, sh.read_off)) die("Error: cannot open %s for reading\n", R.reads_fn.c_str());
    HostBatch b;
    BamWriter::Encoded shard_e;
    // the worker iterates over first-segment groups (long_spanning_reads.cpp:2706-2765); segments to the right are
    // looked up by id (look_right_for_hit_group :87-163; the kernel stops at the first empty segment as it does)
    std::vector<Hit> g;
    for (;;) {
        // first-segment groups of the contig and the spliced stream, merged by id (:2706-2765)
        uint32_t id = st[0].next_group_id();
        const uint32_t sid = sst.empty() ? 0 : sst[0].next_group_id();
        if (sid && (id == 0 || sid < id)) id = sid;
        if (id == 0) break;
        Read rd;
        if (!reads.get(id, rd)) die("Error: could not get read # %d from stream\n", (int)id);
        for (int s = 0; s < nseg; ++s) {
            g.clear();
            take_group(st[(size_t)s], id, g);           // (the first segment's stream has no smaller id left: id is its next, or the spliced stream's)
            if ((size_t)s < sst.size()) take_group(sst[(size_t)s], id, g);       // spliced hits are appended after the contig hits (:125-147, :2738-2744)
            for (auto& h : g) b.hits.push_back(h.h32);
            b.seg_off.push_back((uint32_t)b.hits.size());
        }
        b.text.add(rd);
        b.reads.push_back(std::move(rd));
        if ((size_t)b.text.n() >= R.plan.batch_reads) flush_host_batch(R, k, gpu, b, shard_e);
    }
    flush_host_batch(R, k, gpu, b, shard_e);
    if (R.plan.parts == 1) R.planner.deliver(k, std::move(shard_e));
}

// JoinSegmentsWorker (long_spanning_reads.cpp:2669-2845) for one shard
static void run_shard(Run& R, size_t k) {
    struct AtExit { long long t; ~AtExit() { g_work.add(0, t); } } at_exit{WorkClock::now()};
    trace(k, "start");
    Gpu& gpu = *R.gpus[k % R.gpus.size()];
    if (R.dev_ingest) {                                  // the host reads the shard's reads only, or nothing at all
        Ingested in;
        ingest_on_device(R, k, gpu, in);
        if (in.rc == THJ_OK) {
            if (in.dev) finish_ingested_shard(R, k, gpu, in);
            else if (R.plan.parts == 1) R.planner.deliver(k, BamWriter::Encoded());
            return;
        }
        if (in.rc != THJ_EFALLBACK) die("Error: %s\n", thj_last_error());
        static std::atomic<bool> told{false};
        g_host_ingest_shards.fetch_add(1);
        if (!told.exchange(true)) fprintf(stderr, "\tdevice-side ingest not possible (%s); reading on the host\n", thj_last_error());
    }
    run_shard_host_readers(R, k, gpu);
}

static int real_main(int argc, char** argv) {
    fprintf(stderr, "long_spanning_reads (MI355X-native, %s)\n--------------------------------------------\n", thj_version());
    Opts o;
    int rc = parse_options(argc, argv, o, print_usage);
    if (rc) return rc;
    std::vector<std::string> pos;
    for (int i = optind; i < argc; ++i) pos.push_back(argv[i]);
    if (pos.size() < 8) { print_usage(); return 1; }
    if (o.color) die("Error: colour-space reads are not supported by this build\n");
    o.p.fusion_search = o.fusion_search ? 1 : 0;
    std::vector<std::string> spliced_segs;
    if (pos.size() >= 9) spliced_segs = split(pos[8], ',');
    const std::vector<std::string> segs = split(pos[7], ',');
    if (segs.empty()) { fprintf(stderr, "No hits to process, exiting\n"); return 0; }           // long_spanning_reads.cpp:2883-2887
    const std::string& reads_fn = pos[1];
    const std::string& out = pos[6];

    // the reference is read on its own thread(s) while the HIP runtime starts (the device count is its first call, ~50 ms)
    RefTable rt;
    rt.load_sam_header(o.sam_header);
    fprintf(stderr, "Loading reference sequences...\n");
    std::future<void> fasta_loaded = std::async(std::launch::async, [&rt, &pos]() { rt.load_reference(pos[0], pos[6]); });
    // contexts per GPU: two on a single GPU (measured 2.4 -> 2.0 s for segment_juncs on 8 M pairs).  Three where there is enough to
    // overlap: a shard's inflate launch is ~1500 members, a quarter of what the GPU holds, so three contexts' launches overlap
    // (1.22 -> 1.09 s per side on 10 M pairs; segment_juncs, with ten times larger shards, keeps two) -- but a context costs ~50 ms to
    // start -- its stream, its first launches and allocations -- and a side of 10 M pairs, 1.4 GB of maps, is through in 0.4 s: two
    // contexts there, 2.22-2.26 s against 2.33-2.48 for the three processes; at 40 M pairs three, 4.14-4.39 s against 4.50-4.62.
    const int64_t in_bytes = input_bytes(reads_fn, segs);
    std::vector<std::unique_ptr<Gpu>> gpus = start_contexts(in_bytes > (3ll << 30) ? 3 : 2, getenv("THJ_NO_WARM") ? 0 : THJ_WARM_SPAN | THJ_WARM_INGEST | THJ_WARM_BAMOUT, g_timer);
    const int n_gpus = (int)gpus.size();
    fasta_loaded.get();
    fprintf(stderr, "        reference sequences loaded.\n");
    g_timer.lap("options + reference FASTA");

    SpanSets sets = load_span_sets(rt, pos, o.fusion_search);
    for (auto& f : segs) register_targets(f, rt);        // (the contig maps only: a junction-db map's targets are no contigs)
    rt.freeze();
    {   // junctions on contigs the device genome does not know cannot be closed anyway: drop them
        std::vector<thj_junction> keep;
        for (auto& j : sets.juncs) if (j.ref_id >= 1 && j.ref_id <= rt.names.size() && (j.right - j.left) < (1u << 29)) keep.push_back(j);
        sets.juncs.swap(keep);
    }
    g_timer.lap("junction / indel lists");

    // BAM segment maps mapped for the device-side ingest.  Junction-db maps too: all of a run come from one bowtie index, so their
    // headers name the same targets, and those names are tokenised here, once, into the table the device resolves a record's
    // target with.  Anything else -- a map that is no BAM, headers that differ, more junction-db maps than segments -- and the
    // host readers take the run.
    std::vector<std::unique_ptr<BamFile>> bams, sbams;
    std::vector<thj_juncdb_target> juncdb;
    bool dev_ingest = !getenv("THJ_HOST_INGEST") && spliced_segs.size() <= segs.size();
    for (size_t s = 0; s < segs.size() && dev_ingest; ++s) { bams.emplace_back(new BamFile()); if (!bams.back()->open(segs[s], rt)) dev_ingest = false; }
    for (size_t s = 0; s < spliced_segs.size() && dev_ingest; ++s) {
        sbams.emplace_back(new BamFile());
        if (!sbams.back()->open(spliced_segs[s], rt) || sbams.back()->targets != sbams[0]->targets) dev_ingest = false;
    }
    if (dev_ingest && !sbams.empty()) {
        int bad = 0;
        for (const std::string& t : sbams[0]->targets) { juncdb.push_back(juncdb_target_from_name(t, rt, bad < 1)); bad += juncdb.back().type == THJ_JUNCDB_INVALID; }
        if (bad > 1) fprintf(stderr, "Warning: %d malformed junction-db targets in all\n", bad);
        if (juncdb.empty()) { thj_juncdb_target none; memset(&none, 0, sizeof none); none.type = THJ_JUNCDB_INVALID; juncdb.push_back(none); }     // (a header without targets: there is a table all the same)
    }
    if (!dev_ingest) { bams.clear(); sbams.clear(); juncdb.clear(); }
    // the reads file too when it is an (unaligned) BAM: its members are then inflated on the device with the maps' and the read
    // records come back ready to be copied into the output (THJ_HOST_READS=1: the host ReadStream instead)
    BamFile reads_bam;
    const bool dev_reads = dev_ingest && !getenv("THJ_HOST_READS") && reads_bam.open(reads_fn, rt);
    const RunPlan plan = plan_run(o, reads_fn, segs, spliced_segs, in_bytes, dev_ingest, n_gpus);
    const size_t S = plan.shards.size();
    fprintf(stderr, "\t%d read-id shard%s, %d host CPUs, %d GPU context%s\n", (int)S, S > 1 ? "s" : "", plan.hw, n_gpus, n_gpus > 1 ? "s" : "");
    // ... and with the reads on the device -- and one output file -- the records are built and deflated there too (thj_span_bam_encode,
    // thj_bgzf_deflate): the host wraps the members and writes them.  THJ_HOST_BAM=1 (or a zlib level asked for with
    // THJ_BGZF_LEVEL): the host encoder.
    const bool dev_out = dev_reads && !getenv("THJ_HOST_BAM") && !getenv("THJ_BGZF_LEVEL") && plan.parts == 1;

    std::vector<std::unique_ptr<BamWriter>> bws;
    for (int k = 0; k < plan.parts; ++k) {                      // -p N: <base>{0..N-1}.bam (long_spanning_reads.cpp:3056-3064)
        const std::string fn = plan.parts == 1 ? out : out.substr(0, out.size() >= 4 ? out.size() - 4 : out.size()) + std::to_string(k) + ".bam";
        bws.emplace_back(new BamWriter());
        if (!bws.back()->open(fn, rt, fn + ".index")) die("Error: could not create BAM file %s!\n", fn.c_str());
    }
    Pool pool;
    Planner planner(pool, S, plan.lookahead);
    Run R{o, rt, reads_fn, segs, spliced_segs, sets, plan, gpus, bams, sbams, juncdb, reads_bam, dev_ingest, dev_reads, dev_out, bws, pool, planner, {}};
    if (dev_out) for (const std::string& name : rt.names) R.tid_of_ref.push_back(bws[0]->tid_of(name));

    std::atomic<size_t> next{0};
    auto feed = [&]() {
        for (;;) {
            const size_t k = next.fetch_add(1);
            if (k >= S) { if (!getenv("THJ_NO_DRAIN")) thj_pinned_drain(); return; }     // no shard left to start: page-locked buffers go back as they come free, beside the shards still running
            if (plan.parts == 1) planner.wait_for_turn(k);
            run_shard(R, k);
        }
    };
    if (plan.parts == 1) pool.start(plan.pool_threads);
    std::vector<std::thread> th;
    for (size_t t = 0; t < std::min<size_t>((size_t)plan.feeders, S); ++t) th.emplace_back(feed);
    if (plan.parts == 1) planner.write_in_order(*bws[0]);
    for (auto& t : th) t.join();
    pool.finish();
    g_timer.lap("ingest + stitch + encode + write (all shards)");
    fprintf(stderr, "\tshards read on the host because the device-side ingest declined them: %lld\n", g_host_ingest_shards.load());
    if (dev_out) fprintf(stderr, "\tBAM records and BGZF members made on the device for %lld shard%s, on the host for %lld\n", R.dev_out_shards.load(), R.dev_out_shards.load() == 1 ? "" : "s", R.host_out_shards.load());
    for (auto& bw : bws) bw->close();
    g_timer.lap("BAM close");
    g_timer.report();
    thj_ingest_timing_report();
    { static const char* const nm[4] = {"shards (ingest + merge + device + encode)", "  waiting for the GPU's lock", "  device calls (upload, stitch, download)", "  record encoding"}; g_work.report(nm); }
    // Everything is written and closed.  Leave without running the exit handlers or freeing the contexts: tearing the HIP
    // runtime down after a context has been used takes ~0.2 s that nobody is waiting for.
    rt.finish_cache();                 // (the packed-genome cache's writer, when this process was the one to pack the reference)
    finish_outputs_complete(0);
}

int main(int argc, char** argv) { return run_with_handoff(argc, argv, real_main); }
