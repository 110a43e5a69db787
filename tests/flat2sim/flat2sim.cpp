// TEST-ONLY: flat2_read (thj_core.h) against the enumeration it stands for -- gaps_prepare, and unless that asks for the rescue
// indels_enumerate and gaps_enumerate -- on generated reads of at most two hits a segment, compiled for the CPU.  The reads come
// from a seed over a small set of coordinates, so that every relation between two hits (abutting, at intron distance for the next
// segment or the one after, just outside either range, overlapping, an indel's discrepancy at and one past the limits) occurs
// often.  Per read: the two task multisets word for word, the counts, the rescue verdict and `size`.
//   flat2sim [seed [reads]]   prints "FLAT2SIM reads N differ D <category> <count> ..." and fails when a read differs or a category
//   has fewer than 100 reads.
//   flat2sim pairs [seed [reads]]   the index word of the indel tasks, which the device never materialises (its sink only asks "any
//   task?"): reads whose hits lie a few bases off one diagonal, so that a segment pair has two and more candidate pairs; per read the
//   indel tasks of flat2_read and of indels_enumerate as sets, and every word against the lists themselves.  Prints "FLAT2PAIRS
//   reads N differ D two_pairs M four_pairs M antisense M second_pair M" and fails when a read differs or a count is below 100.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../tophat_amd/csrc/thj_core.h"

using namespace thj;

typedef std::array<uint32_t, 4> Task;

struct RefSink {               // the task words of the kernels' queue sink (QueueSink in thj_segjuncs.hip), hit indices as the view has them
    std::vector<Task> tasks;
    int n_windows = 0, n_indels = 0, n_del = 0, n_ins = 0, n_anti = 0;
    void window(uint32_t ref, int32_t wl, int32_t wr, bool anti, int start, int slen) {
        ++n_windows;
        tasks.push_back(Task{task_window_word(anti, start, slen), ref, (uint32_t)wl, (uint32_t)wr});
    }
    void indel(int i, uint32_t lidx, uint32_t ridx, int li, int ri, bool anti, int plen, bool is_del) {
        ++n_indels;
        if (is_del) ++n_del; else ++n_ins;
        if (anti) ++n_anti;
        tasks.push_back(Task{task_indel_word(anti, is_del, i, plen), lidx, ridx, (uint32_t)li | ((uint32_t)ri << 16)});
    }
};
struct VecEmit {
    std::vector<Task> tasks;
    void task(bool ok, uint32_t a, uint32_t b, uint32_t c, uint32_t d) { if (ok) tasks.push_back(Task{a, b, c, d}); }
};

struct Rng {                   // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    int below(int n) { return (int)(next() % (uint64_t)n); }
    bool chance(int pct) { return below(100) < pct; }
};

enum { C_ABUT, C_S1, C_S2, C_BOTH, C_SECOND, C_DEL, C_INS, C_ANTI, C_RESCUE, C_MULTI, C_SINGLE, C_N };
static const char* const CAT[C_N] = {"abutting_partner", "s1_window", "s2_window", "both_candidates", "second_hit_window", "deletion_pair", "insertion_pair",
                                     "antisense_pair", "rescue", "max_seg_multihits_return", "single_segment_return"};

static const int NS = 4;
static const int32_t MIRROR = 1 << 20;         // an antisense hit lies at MIRROR - (its place in the read's own frame)

// flat2_read's (a | b << 16) against indels_enumerate's (li | ri << 16), and both against what the words mean: the task's hit of
// segment i is hit li of that segment's list, its hit of segment i + 1 hit ri of the next (whichever is `left` after the swap)
static int pairs_main(uint64_t seed, int n_reads) {
    Rng rng{seed};
    long differ = 0, two = 0, four = 0, n_anti = 0, second = 0;
    for (int r = 0; r < n_reads; ++r) {
        Params p;
        memset(&p, 0, sizeof p);
        p.segment_length = 25; p.segment_mismatches = 2;
        p.min_segment_intron = 50; p.max_segment_intron = 400;
        p.max_insertion_length = rng.chance(50) ? 3 : 6; p.max_deletion_length = 3;
        p.bowtie2 = 1; p.max_seg_multihits = 40;
        const int L = p.segment_length;
        const int nseg = 3 + rng.below(2);
        const int rl = nseg * L;
        const bool anti = rng.chance(50);
        const uint32_t base = (uint32_t)rng.below(57);
        std::vector<Hit> hits(base + 2 * NS);
        uint32_t so[NS + 1], n[NS];
        Hit h[NS][2];
        memset(h, 0, sizeof h);
        uint32_t at = base;
        const int32_t origin = 5000 + rng.below(40);
        for (int s = 0; s < NS; ++s) {
            so[s] = at;
            n[s] = 0;
            if (s >= nseg) continue;
            const int k = rng.chance(85) ? 2 : 1;
            for (int a = 0; a < k; ++a) {
                const int32_t x = origin + s * L + rng.below(9) - 4;      // up to four bases off the diagonal, either way
                const bool hanti = rng.chance(4) ? !anti : anti;
                Hit q;
                q.ref_id = rng.chance(4) ? 2 : 1;
                q.left = hanti ? MIRROR - (x + L) : x;
                q.right = q.left + L;
                q.meta = (hanti ? 1u : 0u) | (s == nseg - 1 ? 2u : 0u) | ((uint32_t)rng.below(3) << 8) | ((uint32_t)L << 24);
                hits[at++] = q;
                h[s][a] = q;
                ++n[s];
            }
        }
        so[NS] = at;
        ReadView v;
        memset((void*)&v, 0, sizeof v);
        v.hits = hits.data(); v.so = so; v.nseg = nseg; v.W = 1; v.rl = rl; v.n_mate = 0; v.n_plist = -1;
        RefSink ref_sink;
        indels_enumerate(p, v, ref_sink);
        VecEmit em;
        const FlatResult res = flat2_read<NS>(p, nseg, so, n, h, rl, 0, em);
        std::vector<Task> mine;
        for (const Task& t : em.tasks) if (task_is_indel(t[0])) mine.push_back(t);
        std::sort(mine.begin(), mine.end());
        std::sort(ref_sink.tasks.begin(), ref_sink.tasks.end());
        bool same = !res.rescue && mine == ref_sink.tasks && std::adjacent_find(mine.begin(), mine.end()) == mine.end() && res.n_indels == (int)mine.size();
        int per_pair[NS] = {0, 0, 0, 0};
        for (const Task& t : mine) {
            const int i = task_indel_i(t[0]);
            const bool tanti = task_anti(t[0]);
            const uint32_t li = t[3] & 0xFFFFu, ri = t[3] >> 16;
            const uint32_t of_i = tanti ? t[2] : t[1], of_next = tanti ? t[1] : t[2];
            if (i < 0 || i + 2 >= nseg || li >= n[i] || ri >= n[i + 1] || of_i != so[i] + li || of_next != so[i + 1] + ri || hit_anti(hits[of_i]) != tanti) { same = false; break; }
            ++per_pair[i];
            if (tanti) ++n_anti;
            if (i > 0) ++second;
        }
        for (int i = 0; i < NS; ++i) { if (per_pair[i] >= 2) ++two; if (per_pair[i] == 4) ++four; }
        if (!same && ++differ <= 5) fprintf(stderr, "read %d differs: %zu / %zu indel tasks\n", r, mine.size(), ref_sink.tasks.size());
    }
    printf("FLAT2PAIRS reads %d differ %ld two_pairs %ld four_pairs %ld antisense %ld second_pair %ld\n", n_reads, differ, two, four, n_anti, second);
    if (differ) { fprintf(stderr, "%ld reads differ\n", differ); return 1; }
    if (two < 100 || four < 100 || n_anti < 100 || second < 100) { fprintf(stderr, "a count is below 100\n"); return 2; }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "pairs")) return pairs_main(argc > 2 ? strtoull(argv[2], nullptr, 10) : 15, argc > 3 ? atoi(argv[3]) : 20000);
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 15;
    const int n_reads = argc > 2 ? atoi(argv[2]) : 120000;
    Rng rng{seed};
    long cat[C_N] = {0};
    long differ = 0;
    for (int r = 0; r < n_reads; ++r) {
        Params p;
        memset(&p, 0, sizeof p);
        p.segment_length = 25; p.segment_mismatches = 2;
        p.min_segment_intron = 50; p.max_segment_intron = 400;
        p.max_insertion_length = 3; p.max_deletion_length = 3;
        p.bowtie2 = rng.chance(50) ? 1 : 0;
        p.max_seg_multihits = 1 + rng.below(3);
        const int L = p.segment_length;
        const int nseg = 1 + rng.below(NS);
        const int rl = rng.chance(60) ? nseg * L : 20 + rng.below(81);
        const int n_mate = rng.chance(50) ? 0 : 1 + rng.below(3);
        const bool anti = rng.chance(50);
        const uint32_t ref = 1 + (uint32_t)rng.below(2);
        // the gap in front of a hit, from a list that holds every edge: 0 abuts; the intron range and one base outside it on either side, for
        // the next segment and (a segment further on) the one after; an overlap; discrepancies of an indel pair up to one past the limits
        static const int GAPS[] = {0, 0, 0, 0, 0, 0, 49, 50, 51, 399, 400, 24, 25, 26, 74, 75, 374, 375, 376, 424, 425, -5, 1, 2, 3, 4, -1, -2, -3, -4, 120};
        const int n_gaps = (int)(sizeof GAPS / sizeof GAPS[0]);
        const uint32_t base = (uint32_t)rng.below(57);               // the read's first hit in the batch
        std::vector<Hit> hits(base + 2 * NS);
        uint32_t so[NS + 1], n[NS];
        Hit h[NS][2];
        memset(h, 0, sizeof h);
        uint32_t at = base;
        int32_t cursor = 5000 + rng.below(40);                       // where the next segment would start if the read lay ungapped
        for (int s = 0; s < NS; ++s) {
            so[s] = at;
            n[s] = 0;
            if (s >= nseg) continue;
            const int k = rng.chance(12) ? 0 : rng.chance(45) ? 1 : 2;
            int first_gap = 0;
            for (int a = 0; a < k; ++a) {
                const int gap = GAPS[rng.below(n_gaps)];
                if (a == 0) first_gap = gap;
                const int32_t x = cursor + gap;
                const bool hanti = rng.chance(8) ? !anti : anti;
                Hit q;
                q.ref_id = rng.chance(8) ? 3 - ref : ref;
                q.left = hanti ? MIRROR - (x + L) : x;
                q.right = q.left + L;
                const bool end = s == nseg - 1 || (s == 0 && rng.chance(25));
                q.meta = (hanti ? 1u : 0u) | (end ? 2u : 0u) | ((uint32_t)rng.below(3) << 8) | ((uint32_t)L << 24);
                hits[at++] = q;
                h[s][a] = q;
                ++n[s];
            }
            cursor += L + (rng.chance(70) ? first_gap : 0);
        }
        so[NS] = at;

        // ---- the reference: the loops over the lists
        ReadView v;
        memset((void*)&v, 0, sizeof v);
        v.hits = hits.data(); v.so = so; v.nseg = nseg; v.W = 1; v.rl = rl; v.n_mate = n_mate; v.n_plist = -1;
        RefSink ref_sink;
        bool wants = false;
        const bool do_gaps = gaps_prepare(p, v, wants);
        const bool to_rescue = do_gaps && wants;
        if (!to_rescue) {
            indels_enumerate(p, v, ref_sink);
            if (do_gaps) gaps_enumerate(p, v, ref_sink);
        }
        // ---- the straight-line form
        VecEmit em;
        const FlatResult res = flat2_read<NS>(p, nseg, so, n, h, rl, n_mate, em);

        std::sort(ref_sink.tasks.begin(), ref_sink.tasks.end());
        std::sort(em.tasks.begin(), em.tasks.end());
        const bool same = ref_sink.tasks == em.tasks && res.n_windows == ref_sink.n_windows && res.n_indels == ref_sink.n_indels &&
                          res.rescue == to_rescue && res.size == v.size;
        if (!same) {
            if (++differ <= 5)
                fprintf(stderr, "read %d differs: nseg %d rl %d mates %d counts %u %u %u %u; tasks %zu / %zu, windows %d / %d, indels %d / %d, rescue %d / %d, size %d / %d\n",
                        r, nseg, rl, n_mate, n[0], n[1], n[2], n[3], em.tasks.size(), ref_sink.tasks.size(), res.n_windows, ref_sink.n_windows,
                        res.n_indels, ref_sink.n_indels, (int)res.rescue, (int)to_rescue, res.size, v.size);
        }

        // ---- what the read was, told from its lists alone
        bool c[C_N] = {false};
        c[C_DEL] = ref_sink.n_del > 0; c[C_INS] = ref_sink.n_ins > 0; c[C_ANTI] = ref_sink.n_anti > 0;
        c[C_RESCUE] = to_rescue;
        c[C_SINGLE] = v.size == 1 && n[0] > 0 && hit_end(h[0][0]);
        bool multi = false;
        for (int s = 0; s < v.size; ++s) if (p.bowtie2 && (int)n[s] > p.max_seg_multihits) multi = true;
        c[C_MULTI] = do_gaps && !to_rescue && multi;
        if (do_gaps && !to_rescue && !multi)
            for (int s = 0; s + 1 < v.size; ++s)
                for (uint32_t a = 0; a < n[s]; ++a) {
                    const Hit bh = h[s][a];
                    const bool banti = hit_anti(bh);
                    bool found = false;
                    int n1 = 0, n2 = 0, last1 = -1, last2 = -1;
                    for (uint32_t b = 0; b < n[s + 1]; ++b) {
                        const Hit rh = h[s + 1][b];
                        if (banti != hit_anti(rh) || bh.ref_id != rh.ref_id) continue;
                        if (banti ? rh.right == bh.left : bh.right == rh.left) found = true;
                        const int dist = banti ? bh.left - rh.right : rh.left - bh.right;
                        if (dist >= p.min_segment_intron && dist < p.max_segment_intron) { ++n1; last1 = (int)b; }
                    }
                    for (uint32_t b = 0; s + 2 < v.size && b < n[s + 2]; ++b) {
                        const Hit rh = h[s + 2][b];
                        if (banti != hit_anti(rh) || bh.ref_id != rh.ref_id) continue;
                        const int dist = banti ? bh.left - rh.right : rh.left - bh.right;
                        if (dist >= p.min_segment_intron + L && dist < p.max_segment_intron + L) { ++n2; last2 = (int)b; }
                    }
                    const int start = (s + 1) * L - 8;
                    if (found) { c[C_ABUT] = true; continue; }
                    if (rl - start < 0) continue;
                    if (n1 > 0 && n2 == 0) c[C_S1] = true;
                    if (n2 > 0) c[C_S2] = true;
                    if (n1 > 0 && n2 > 0) c[C_BOTH] = true;
                    if ((n1 > 0 || n2 > 0) && (a == 1 || (n2 > 0 ? last2 : last1) == 1)) c[C_SECOND] = true;
                }
        for (int k = 0; k < C_N; ++k) cat[k] += c[k] ? 1 : 0;
    }
    printf("FLAT2SIM reads %d differ %ld", n_reads, differ);
    bool thin = false;
    for (int k = 0; k < C_N; ++k) { printf(" %s %ld", CAT[k], cat[k]); if (cat[k] < 100) thin = true; }
    printf("\n");
    if (differ) { fprintf(stderr, "%ld reads differ\n", differ); return 1; }
    if (thin) { fprintf(stderr, "a category has fewer than 100 reads\n"); return 2; }
    return 0;
}
