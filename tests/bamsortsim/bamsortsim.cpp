// TEST-ONLY: the order thj_bam_stream_sort gives a stream's records (tophat_amd/csrc/thj_bamsort_core.h: the record head at any alignment,
// bam1_lt's key, the bits a sort looks at, the block cut, a record's block, the tail bit's placement), compiled for the CPU.  The loops
// around the core's decisions are the plain ones of the steps the kernels of thj_bamsort.hip take: a stable sort of (key, index) over the
// key's low bits, run and segment heads in sorted order, their numbers by prefix sums, a first reverse-strand entry per segment, the
// count of tail-0 entries before every entry, tail_place.
//
//     bamsortsim [time]
// stdin, any number of inputs:
//     C <max_mem> <n>
//     <tid> <pos> <strand> <size>        n lines: a record in stream order, size = 4 + block_size
// and what is printed per input:
//     B <blocks the reference would have written>
//     O <input record number> ...        in output order
//     (X <record> <why>                  instead of both: a record that does not fill its size, or a position the keys do not order alike)
// With `time` the orders are not printed and stderr gets the milliseconds spent ordering (one core; for scale beside the device's).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../tophat_amd/csrc/thj_bamsort_core.h"

struct Rec { int32_t tid, pos; uint32_t strand, size; };

static void wr32(uint8_t* p, uint32_t v) { for (int k = 0; k < 4; ++k) p[k] = (uint8_t)(v >> (8 * k)); }

// -> false: a record was refused (printed)
static bool order_of(const std::vector<Rec>& recs, uint64_t max_mem, std::vector<uint32_t>& perm, int64_t& n_blocks) {
    const uint32_t n = (uint32_t)recs.size();
    // the stream's record heads, back to back at whatever alignment the sizes give (the first at an odd byte), 20 bytes each as head_of reads
    std::vector<uint64_t> off(n + 1, 0);
    for (uint32_t i = 0; i < n; ++i) off[i + 1] = off[i] + recs[i].size;
    std::vector<uint8_t> stream((size_t)off[n] + 1 + 20, 0);
    for (uint32_t i = 0; i < n; ++i) {
        uint8_t* p = stream.data() + 1 + off[i];
        wr32(p, recs[i].size - 4u); wr32(p + 4, (uint32_t)recs[i].tid); wr32(p + 8, (uint32_t)recs[i].pos); wr32(p + 16, (recs[i].strand ? 0x10u : 0u) << 16 | 0x400u << 16);
    }
    bsort::Cut cut(max_mem);
    std::vector<uint32_t> block_start{0u};
    for (uint32_t i = 0; i < n; ++i) if (cut.add(recs[i].size)) block_start.push_back(i + 1u);
    n_blocks = cut.n_blocks();
    // keys
    std::vector<uint64_t> key(n); std::vector<uint32_t> val(n);
    bool neg = false; uint32_t max_tid = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const bsort::Head h = bsort::head_of(stream.data() + 1 + off[i]);
        if (!bsort::head_ok(h, recs[i].size)) { printf("X %u size\n", i); return false; }
        if (!bsort::pos_ok(h.pos)) { printf("X %u pos\n", i); return false; }
        if (h.tid < 0) neg = true; else if ((uint32_t)h.tid > max_tid) max_tid = (uint32_t)h.tid;
        key[i] = bsort::block_key(h.tid, h.pos); val[i] = i | (h.strand << 31);
    }
    // the radix sort looks at the low key_bits bits only
    const int bits = bsort::key_bits(neg, max_tid);
    const uint64_t mask = bits >= 64 ? ~0ull : ((1ull << bits) - 1ull);
    std::vector<uint32_t> ord(n);
    for (uint32_t i = 0; i < n; ++i) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return (key[a] & mask) < (key[b] & mask); });
    std::vector<uint64_t> skey(n); std::vector<uint32_t> sval(n);
    for (uint32_t i = 0; i < n; ++i) { skey[i] = key[ord[i]]; sval[i] = val[ord[i]]; }
    perm.assign(n, 0);
    if (n_blocks == 1) { for (uint32_t i = 0; i < n; ++i) perm[i] = sval[i] & 0x7FFFFFFFu; return true; }
    const uint32_t nb = (uint32_t)block_start.size();
    std::vector<uint32_t> run(n), seg(n), run_start(n + 1, 0), first_rev(n, 0xFFFFFFFFu), tail0(n + 1, 0), z(n + 1, 0);
    uint32_t r = 0, s = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const bool rh = i == 0 || skey[i] != skey[i - 1];
        const bool sh = rh || bsort::block_of(block_start.data(), nb, sval[i] & 0x7FFFFFFFu) != bsort::block_of(block_start.data(), nb, sval[i - 1] & 0x7FFFFFFFu);
        if (rh) { if (i) ++r; run_start[r] = i; }
        if (sh && i) ++s;
        run[i] = r; seg[i] = s;
    }
    if (n) run_start[r + 1] = n;
    for (uint32_t i = 0; i < n; ++i) if ((sval[i] >> 31) && i < first_rev[seg[i]]) first_rev[seg[i]] = i;
    for (uint32_t i = 0; i < n; ++i) tail0[i] = i < first_rev[seg[i]] ? 1u : 0u;
    for (uint32_t i = 0; i < n; ++i) z[i + 1] = z[i] + tail0[i];
    // (the same bit from the walk along a segment, the way the rule is told)
    uint32_t seen = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (i == 0 || seg[i] != seg[i - 1]) seen = 0;
        if (bsort::tail_step(seen, sval[i] >> 31) != (tail0[i] ^ 1u)) { printf("X %u tail\n", i); return false; }
    }
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t a = run_start[run[i]], e = run_start[run[i] + 1];
        perm[bsort::tail_place(a, e, i, tail0[i] ^ 1u, z[a], z[i], z[e])] = sval[i] & 0x7FFFFFFFu;
    }
    return true;
}

int main(int argc, char** argv) {
    const bool timing = argc > 1 && !strcmp(argv[1], "time");
    char c;
    unsigned long long max_mem; unsigned n;
    double ms = 0;
    while (scanf(" %c %llu %u", &c, &max_mem, &n) == 3 && c == 'C') {
        std::vector<Rec> recs(n);
        for (unsigned i = 0; i < n; ++i) {
            long tid, pos; unsigned strand, size;
            if (scanf("%ld %ld %u %u", &tid, &pos, &strand, &size) != 4) { fprintf(stderr, "bamsortsim: short input\n"); return 2; }
            recs[i] = Rec{(int32_t)tid, (int32_t)pos, strand, size};
        }
        std::vector<uint32_t> perm; int64_t nb = 1;
        const auto t0 = std::chrono::steady_clock::now();
        const bool ok = order_of(recs, max_mem, perm, nb);
        ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (!ok || timing) continue;
        printf("B %lld\nO", (long long)nb);
        for (uint32_t p : perm) printf(" %u", p);
        printf("\n");
    }
    if (timing) fprintf(stderr, "bamsortsim: %.3f ms\n", ms);
    return 0;
}
