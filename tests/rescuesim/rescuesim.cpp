// TEST-ONLY: flat_rescue_read (thj_core.h), the per-read body of thj_k_sj_rescue_flat, against what it stands for -- rescue_scan for
// every mate hit, then flat_rescue, as tests/hostsim does it -- on generated reads, compiled for the CPU.  The reads come from a seed
// over a small set of coordinates on two short contigs, both strands: 2-4 kept segments with one hit in the first, lengths 50-100,
// 0-3 mate hits (0 and 3 are the neighbours thj_k_sj_flat does not list; 3 runs both sides with room for three), the read's last
// bases planted in a mate hit's flank at every distance from the first-segment hit that matters.  The new function is handed the
// packed 32-byte entry, and every array it reads lies in a heap block of its exact size.  Per read: the task words in order, the
// pair count and the window count.
//   rescuesim [seed [reads]]   prints "RESCUESIM reads N differ D <category> <count> ..." and fails when a read differs or a category
//   has fewer than 100 reads.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../tophat_amd/csrc/thj_core.h"

using namespace thj;

typedef std::array<uint32_t, 4> Task;
struct VecEmit {
    std::vector<Task> tasks;
    void task(bool ok, uint32_t a, uint32_t b, uint32_t c, uint32_t d) { if (ok) tasks.push_back(Task{a, b, c, d}); }
};
struct OneLane { bool any(bool x) const { return x; } };       // a read at a time: the wave is this lane

struct Rng {                   // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    int below(int n) { return (int)(next() % (uint64_t)n); }
    bool chance(int pct) { return below(100) < pct; }
};

enum { C_COMPAT, C_CONTIG, C_STRAND, C_BREAK, C_CLIP, C_ABUT, C_NEAR, C_FAR, C_SIZE2, C_SIZE3, C_ANTI, C_TWO, C_N };
static const char* const CAT[C_N] = {"compatible_pair", "other_contig", "same_strand", "break_then_good", "flank_clipped", "abutting_pseudo_hit",
                                     "below_min_intron", "at_or_above_max_intron", "size2_window", "size3_window", "antisense_first_hit", "two_mates_windows"};

static const int N_CONTIG = 2;
static const int32_t CLEN[N_CONTIG] = {1500, 1100};
static const int W = 2;        // plane words a read: up to 128 bases

// the reference: hostsim's flat_path after flat_read asked for the rescue
template <int MAXM>
static int reference(const Genome& g, const Params& p, const Hit& bh, int size, int rl, const u64* rp, const Hit* mate, int n_mate,
                     VecEmit& em, int& nw, int32_t (&sc)[2 * MAXM]) {
    Hit mh[MAXM];
    for (int m = 0; m < MAXM; ++m) { mh[m] = Hit{0, 0, 0, 0}; sc[2 * m] = SLOT_NONE; sc[2 * m + 1] = SLOT_NONE; }
    for (int m = 0; m < n_mate; ++m) {
        mh[m] = mate[m];
        if (!rescue_scan(g, p, rp, W, rl, mh[m], sc[2 * m], sc[2 * m + 1]) && sc[2 * m] != SLOT_BREAK) sc[2 * m] = SLOT_UNSCANNED;
    }
    return flat_rescue<MAXM>(p, true, bh, size, rl, mh, n_mate, sc, em, nw);
}

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 16;
    const int n_reads = argc > 2 ? atoi(argv[2]) : 60000;
    Rng rng{seed};

    // ---- the genome: random bases, the device's layout (32-byte blocks of 64 bases, one block behind the last for the funnel)
    std::vector<uint8_t> base[N_CONTIG];
    std::vector<uint32_t> contig_blk(N_CONTIG + 1);
    std::vector<int32_t> contig_len(N_CONTIG);
    uint32_t n_blk = 0;
    for (int c = 0; c < N_CONTIG; ++c) {
        base[c].resize((size_t)CLEN[c]);
        for (int32_t i = 0; i < CLEN[c]; ++i) base[c][(size_t)i] = (uint8_t)rng.below(4);
        contig_blk[(size_t)c] = n_blk; contig_len[(size_t)c] = CLEN[c];
        n_blk += (uint32_t)((CLEN[c] + 63) / 64);
    }
    contig_blk[N_CONTIG] = n_blk;
    std::vector<u64> blocks((size_t)(n_blk + 1) * 4, 0ull);
    for (int c = 0; c < N_CONTIG; ++c)
        for (int32_t i = 0; i < (int32_t)((CLEN[c] + 63) / 64 * 64); ++i) {
            u64* const blk = &blocks[((size_t)contig_blk[(size_t)c] + (size_t)(i >> 6)) * 4];
            const u64 bit = 1ull << (i & 63);
            if (i >= CLEN[c]) { blk[2] |= bit; continue; }
            if (base[c][(size_t)i] & 1) blk[0] |= bit;
            if (base[c][(size_t)i] & 2) blk[1] |= bit;
        }
    const Genome g{blocks.data(), contig_blk.data(), contig_len.data(), N_CONTIG};

    long cat[C_N] = {0};
    long differ = 0;
    for (int r = 0; r < n_reads; ++r) {
        Params p;
        memset(&p, 0, sizeof p);
        p.segment_length = 25; p.segment_mismatches = 2;
        p.min_segment_intron = 50; p.max_segment_intron = 400;
        if (rng.chance(75)) { p.inner_dist_mean = 50; p.inner_dist_std_dev = 20; } else { p.inner_dist_mean = 20; p.inner_dist_std_dev = 50; }
        p.bowtie2 = rng.chance(30) ? 1 : 0;
        p.max_seg_multihits = 1 + rng.below(3);
        const int L = p.segment_length, CL = 15;
        const int part = p.inner_dist_std_dev > p.inner_dist_mean ? p.inner_dist_std_dev - p.inner_dist_mean : 0;
        const int flank = p.inner_dist_mean + p.inner_dist_std_dev;
        const int size = 2 + rng.below(3);
        const int rl = 50 + rng.below(51);
        const int n_mate = rng.chance(8) ? 0 : rng.chance(8) ? 3 : rng.chance(65) ? 1 : 2;
        const bool banti = rng.chance(50);
        const uint32_t ref = 1 + (uint32_t)rng.below(N_CONTIG);
        const int32_t clen = CLEN[ref - 1];
        const bool far = size == 3;

        // ---- the first segment's hit, and where the read's last bases are to be found: at a distance from it out of a list that holds every edge
        static const int DIST[] = {0, 0, 0, 49, 50, 51, 74, 75, 76, 120, 200, 399, 400, 401, 424, 425, 426, -10};
        const int dist = DIST[rng.below((int)(sizeof DIST / sizeof DIST[0]))];
        const bool clip = rng.chance(12);          // ... or at the contig's end, under a mate hit whose flank the end cuts
        Hit bh;
        bh.ref_id = ref;
        bh.left = banti ? clen - 100 - rng.below(300) - L : 100 + rng.below(300);
        bh.right = bh.left + L;
        bh.meta = (banti ? 1u : 0u) | ((uint32_t)rng.below(3) << 8) | ((uint32_t)L << 24);
        int32_t q = banti ? bh.left - dist - CL : bh.right + dist;
        if (clip) q = clen - CL - rng.below(20);
        if (q < 0) q = 0;
        if (q + CL > clen) q = clen - CL;

        // ---- the mate hits: the first (of two: sometimes the second) over q, the others near it; now and then another contig, the same
        // strand, or so close to the contig's start that the reference leaves its mate loop
        std::vector<Hit> mates;
        const uint32_t mate_first = (uint32_t)rng.below(5);       // mate hits of the batch's reads before this one
        for (uint32_t k = 0; k < mate_first; ++k) mates.push_back(Hit{1u + (uint32_t)rng.below(N_CONTIG), 300, 325, (uint32_t)rng.below(2)});
        const bool brk = n_mate >= 2 && rng.chance(25);
        for (int m = 0; m < n_mate; ++m) {
            Hit rh;
            rh.ref_id = rng.chance(10) ? 3 - ref : ref;
            const bool manti = rng.chance(10) ? banti : !banti;
            if (manti) rh.left = q + CL + rng.below(flank - CL + 1);           // its flank: [left - flank, left + part)
            else rh.left = q + part - rng.below(flank - CL + 1) - L;           //            [right - part, right + flank)
            if (clip) rh.left = manti ? clen - rng.below(part + 1) : clen - L - rng.below(40);
            if (rh.left < 0) rh.left = 0;
            if (brk && m == 0) { if (manti) rh.left = rng.below(flank); else if (part) rh.left = rng.below(part) - L; }      // (a sense hit: only where part > 0)
            rh.right = rh.left + L;
            rh.meta = (manti ? 1u : 0u) | ((uint32_t)L << 24);
            mates.push_back(rh);
        }
        Hit* const mate_heap = (Hit*)malloc(mates.size() * sizeof(Hit) + (mates.empty() ? 1 : 0));       // exactly the batch's mate hits up to this read's last
        if (!mates.empty()) memcpy(mate_heap, mates.data(), mates.size() * sizeof(Hit));

        // ---- the read: random bases, its last CL the contig's at q (first-segment hit antisense: their reverse complement), now and then with mismatches
        const uint32_t read = (uint32_t)rng.below(4);             // reads of the batch before this one
        u64* const planes = (u64*)calloc((size_t)(read + 1) * 3 * W, sizeof(u64));
        u64* const rp = planes + (size_t)read * 3 * W;
        std::vector<uint8_t> rb((size_t)rl);
        for (int i = 0; i < rl; ++i) rb[(size_t)i] = (uint8_t)rng.below(4);
        for (int i = 0; i < CL; ++i) rb[(size_t)(rl - CL + i)] = banti ? (uint8_t)(base[ref - 1][(size_t)(q + CL - 1 - i)] ^ 3) : base[ref - 1][(size_t)(q + i)];
        const int n_mm = rng.chance(80) ? 0 : 1 + rng.below(3);
        for (int k = 0; k < n_mm; ++k) rb[(size_t)(rl - CL + rng.below(CL))] ^= (uint8_t)(1 + rng.below(3));
        for (int i = 0; i < rl; ++i) {
            if (rb[(size_t)i] & 1) rp[i >> 6] |= 1ull << (i & 63);
            if (rb[(size_t)i] & 2) rp[W + (i >> 6)] |= 1ull << (i & 63);
        }

        // ---- the entry, packed, in a block of its 32 bytes
        uint32_t w[8];
        flat_rescue_entry_pack(FlatRescueEntry{read, size, bh, rl, n_mate, mate_first}, w);
        uint32_t* const ew = (uint32_t*)aligned_alloc(32, 32);
        memcpy(ew, w, 32);
        const FlatRescueEntry back = flat_rescue_entry_unpack(w);
        bool same = back.read == read && back.size == size && back.rl == rl && back.n_mate == n_mate && back.mate_first == mate_first &&
                    memcmp(&back.bh, &bh, sizeof bh) == 0;

        // ---- both sides
        VecEmit want, got;
        OneLane wave;
        int want_w = 0, got_w = 0, want_p, got_p;
        int32_t sc[6] = {SLOT_NONE, SLOT_NONE, SLOT_NONE, SLOT_NONE, SLOT_NONE, SLOT_NONE};
        if (n_mate <= 2) {
            int32_t s2[4];
            want_p = reference<2>(g, p, bh, size, rl, rp, mate_heap + mate_first, n_mate, want, want_w, s2);
            memcpy(sc, s2, sizeof s2);
            got_p = flat_rescue_read<2>(g, p, true, ew, planes, W, mate_heap, got, wave, got_w);
        } else {
            want_p = reference<3>(g, p, bh, size, rl, rp, mate_heap + mate_first, n_mate, want, want_w, sc);
            got_p = flat_rescue_read<3>(g, p, true, ew, planes, W, mate_heap, got, wave, got_w);
        }
        same = same && want.tasks == got.tasks && want_w == got_w && want_p == got_p && (int)want.tasks.size() == want_w;
        {   // a lane without an entry takes part and gives nothing (the pointer is not read)
            VecEmit none;
            int nw0 = 0;
            if (flat_rescue_read<2>(g, p, false, nullptr, nullptr, W, nullptr, none, wave, nw0) != 0 || nw0 != 0 || !none.tasks.empty()) same = false;
        }
        if (!same && ++differ <= 5)
            fprintf(stderr, "read %d differs: size %d rl %d mates %d anti %d; tasks %zu / %zu, windows %d / %d, pairs %d / %d\n",
                    r, size, rl, n_mate, (int)banti, got.tasks.size(), want.tasks.size(), got_w, want_w, got_p, want_p);

        // ---- what the read was, told from the reference's scans
        bool c[C_N] = {false};
        bool alive = true, in_range[3] = {false, false, false};
        int n_in = 0;
        for (int m = 0; m < n_mate; ++m) {
            const Hit& rh = mate_heap[mate_first + (uint32_t)m];
            if (rh.ref_id != ref) { c[C_CONTIG] = true; continue; }
            if (hit_anti(rh) == banti) { c[C_STRAND] = true; continue; }
            c[C_COMPAT] = true;
            if (!alive) continue;
            if (sc[2 * m] == SLOT_BREAK) {
                alive = false;
                if (m == 0 && n_mate >= 2) {
                    const Hit& nx = mate_heap[mate_first + 1];
                    if (nx.ref_id == ref && hit_anti(nx) != banti && (sc[2] >= 0 || sc[3] >= 0)) c[C_BREAK] = true;
                }
                continue;
            }
            if (sc[2 * m] == SLOT_UNSCANNED) continue;
            const int64_t fl = hit_anti(rh) ? rh.left - flank : rh.right - part;
            if (fl + flank + part > clen) c[C_CLIP] = true;
            const int32_t pl = sc[2 * m + (banti ? 1 : 0)];          // the pseudo-hit on the first-segment hit's strand
            if (pl < 0) continue;
            const int d = banti ? bh.left - (pl + CL) : pl - bh.right;
            if (d == 0 && !far) c[C_ABUT] = true;
            if (d >= 0 && d < p.min_segment_intron + (far ? L : 0)) c[C_NEAR] = true;
            if (d >= p.max_segment_intron + (far ? L : 0)) c[C_FAR] = true;
            if (d >= p.min_segment_intron + (far ? L : 0) && d < p.max_segment_intron + (far ? L : 0)) { in_range[m] = true; ++n_in; }
        }
        if (want_w > 0) {
            c[size == 2 ? C_SIZE2 : C_SIZE3] = true;
            if (banti) c[C_ANTI] = true;
            if (n_mate == 2 && in_range[0] && in_range[1] && want_w == n_in) c[C_TWO] = true;
        }
        for (int k = 0; k < C_N; ++k) cat[k] += c[k] ? 1 : 0;
        free(ew); free(planes); free(mate_heap);
    }
    printf("RESCUESIM reads %d differ %ld", n_reads, differ);
    bool thin = false;
    for (int k = 0; k < C_N; ++k) { printf(" %s %ld", CAT[k], cat[k]); if (cat[k] < 100) thin = true; }
    printf("\n");
    if (differ) { fprintf(stderr, "%ld reads differ\n", differ); return 1; }
    if (thin) { fprintf(stderr, "a category has fewer than 100 reads\n"); return 2; }
    return 0;
}
