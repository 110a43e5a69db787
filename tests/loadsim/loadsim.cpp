// loadsim.cpp -- TEST-ONLY: the load groups of tier 0, the chain join and the finish of a joined hit (thj_span_core.h:
// span_read_contig_pre / contig_finish, chain_entry_fetch, joined_extras) compiled for the CPU and run over planted reads with every
// array -- genome blocks (with the guard block), contig tables, segment offsets, hit records, planes, lengths, quality bytes, junction
// keys and each chain entry -- in a heap block of exactly its size.  The loads of those functions are unconditional: a read of at most 64
// bases fetches "its second piece", a padding entry "its hits", a one-word read its plane words twice.  Under the address sanitizer
// (the loadsim_san target) a load that leaves its array ends the run; a GPU run would not show it.  The records go to a file and
// are compared with the oracle's by tests/test_loadsim_cpu.py.  A program of its own: never loaded into Python, never run on a GPU.
//
//   loadsim <case file> <record file>
// case file (little endian): int32 magic, n_contigs, n_reads, nseg, W, qual_stride; int64 n_block_words, n_hits, n_juncs;
// thj_params; then blocks u64[n_block_words], contig_blk u32[n_contigs + 1], contig_len i32[n_contigs], seg_off u32[n_reads * nseg + 1],
// hits [n_hits] x 32 bytes, planes u64[n_reads * 3 * W], read_len u16[n_reads], quals u8[n_reads * qual_stride], juncs [n_juncs] x 16 bytes
#include "../../include/thj.h"
#include "../../tophat_amd/csrc/thj_core.h"
#include "../../tophat_amd/csrc/thj_span_core.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace thj;

struct VecSink {
    std::vector<OutAln>* v;
    void emit(const OutAln& o) { v->push_back(o); }
    void emit_words(const uint32_t* w) { OutAln o; memcpy(&o, w, sizeof o); v->push_back(o); }
    void set_count(uint32_t, int) {}
};

// a heap block of exactly n elements, filled from the file
template <class T>
static T* take(FILE* f, size_t n) {
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "loadsim: short case file\n"); exit(2); }
    return p;
}

struct Case {
    Genome g; Params p; SpanSets S;
    int32_t n_reads, nseg, W, qual_stride;
    const uint32_t* seg_off; const SpanHit* hits; const u64* planes; const uint16_t* read_len; const uint8_t* quals;
    int64_t n_hits;
};

// one chain entry -> its record, the way thj_k_join_finish / thj_k_join_closure / thj_k_finish do it: the entry in a 32-byte block of
// its own, as a slot of the kernels' lists is.  A padding entry's second half is never written (thj_k_chains): here it holds 0xEE bytes,
// hit numbers far outside the batch -- it is loaded with the first half, one group, and must not be used
static int run_entry(const Case& c, const ChainEntry& ent, bool pad, int order, VecSink& sink, bool& punt) {
    ChainEntry* e = (ChainEntry*)malloc(sizeof(ChainEntry));
    memcpy(e, &ent, sizeof(ChainEntry));
    if (pad) memset((char*)e + 16, 0xEE, 16);
    uint32_t r, meta;
    Q16 rec[2 * CHAIN_MAXSEG];
    RegRead rw;
    int emitted = 0;
    if (chain_entry_fetch(c.hits, c.planes, c.W, e, r, meta, rec, &rw)) {
        SpanHit ch[CHAIN_MAXSEG];
        for (int s = 0; s < CHAIN_MAXSEG; ++s) {
            const Q16 a = rec[2 * s], b = rec[2 * s + 1];
            ch[s].ref_id = a.x; ch[s].left = (int32_t)a.y; ch[s].meta = a.z; ch[s].cigar[0] = a.w;
            ch[s].cigar[1] = b.x; ch[s].cigar[2] = b.y; ch[s].cigar[3] = b.z; ch[s].cigar[4] = b.w;
        }
        const u64* rp = c.planes + (u64)r * (uint32_t)(3 * c.W);
        RAln res;
        int jr = chain_join<true>(c.g, c.p, c.S, ch, meta, rp, c.W, res);
        const bool deferred = jr == LJ_DEFER;
        if (deferred) jr = chain_join<false>(c.g, c.p, c.S, ch, meta, rp, c.W, res);
        if (jr == LJ_PUNT) punt = true;
        if (jr == LJ_OK) {
            Q16 ja, jb, jc;
            joined_pack(res, r, chain_nsegs(meta) == 1, chain_q(meta), chain_k(meta), ja, jb, jc);
            Extras x;
            bool ok;
            if (!deferred) ok = joined_prepare(c.g, c.p, ja, jb, jc, c.planes, c.W, rw, chain_rl(meta), c.quals, c.qual_stride, res, x);      // thj_k_join_finish
            else {                                                                                                                        // thj_k_finish
                RegRead rw2;
                reg_read_load(c.planes + (u64)ja.x * (uint32_t)(3 * c.W), c.W, rw2);
                ok = joined_prepare<0>(c.g, c.p, ja, jb, jc, c.planes, c.W, rw2, (int)c.read_len[ja.x], c.quals, c.qual_stride, res, x);
            }
            if (ok) { emit_aln(sink, r, order, res, x); emitted = 1; }
        }
    }
    free(e);
    return emitted;
}

template <int MS>
static int run(const Case& c, std::vector<std::vector<OutAln>>& outs, long (&n)[6]) {
    for (int32_t r = 0; r < c.n_reads; ++r) {
        VecSink sink{&outs[(size_t)r]};
        const uint32_t* so = c.seg_off + (int64_t)r * c.nseg;
        const u64* rp = c.planes + (int64_t)r * 3 * c.W;
        const uint8_t* q = c.quals + (int64_t)r * c.qual_stride;
        ChainEntry ent;
        int st = span_read_contig<MS>(c.g, c.p, c.hits, so, c.nseg, rp, c.W, c.read_len[r], q, (uint32_t)r, sink, MS <= CHAIN_MAXSEG ? &ent : nullptr);
        if ((st & 0xFF) == SPAN_NEED_CHAIN) {
            ++n[1];
            bool punt = false;
            run_entry(c, ent, false, 0, sink, punt);
            if (punt) return -30;
            continue;
        }
        if ((st & 0xFF) == SPAN_NEED_LEAN) {
            ++n[2];
            SpanHitHead stage[SPAN_MAXSEG];
            st = span_read_lean(c.g, c.p, c.S, c.hits, so, c.nseg, rp, c.W, c.read_len[r], q, (uint32_t)r, stage, sink);
            if (st != SPAN_OK && st != SPAN_INCOMPAT) return -31;
            continue;
        }
        if (st == SPAN_NEED_GENERIC) {
            // a multihit read: its chains as a group of entries in rank order, padded to 1 / 2 / 4 / 8 (thj_k_chains)
            int nsegs = 0;
            while (nsegs < c.nseg && so[nsegs + 1] > so[nsegs]) ++nsegs;
            if (nsegs == 0 || nsegs > CHAIN_MAXSEG || !(c.hits[so[nsegs - 1]].meta & SH_END)) return -32;
            struct HostTab {
                const SpanHit* h0;
                SpanHitHead head(int j) const {
                    const SpanHit& x = h0[j];
                    int right = x.left; int k = (int)(x.meta >> 24); if (k > 5) k = 5;
                    for (int i = 0; i < k; ++i) { const int op = cig_op(x.cigar[i]); if (op == OP_MATCH || op == OP_REF_SKIP || op == OP_DEL) right += (int)cig_len(x.cigar[i]); }
                    return SpanHitHead{x.ref_id, x.left, x.meta, (uint32_t)right};
                }
            } tab{c.hits + so[0]};
            uint32_t off[CHAIN_MAXSEG + 1];
            for (int s = 0; s <= nsegs; ++s) off[s] = so[s] - so[0];
            uint32_t sel[CHAINS_MAX]; int q2[CHAINS_MAX];
            const int k = chains_discover(c.p, tab, off, nsegs, sel, q2);
            if (k == CHAINS_DECLINE) return -33;
            ++n[3];
            int order = 0;
            for (int rank = 0; rank < chains_padded(k); ++rank) {
                ChainEntry e2;
                memset(&e2, 0, sizeof e2);
                e2.read = JOINED_PAD;
                bool pad = true;
                for (int ci = 0; ci < k; ++ci)
                    if (q2[ci] == rank) {
                        e2.read = (uint32_t)r; e2.meta = chain_meta(nsegs, rank, k, c.read_len[r]);
                        for (int s = 0; s < CHAIN_MAXSEG; ++s) e2.hit[s] = so[0] + ((sel[ci] >> (4 * (s < nsegs ? s : 0))) & 15u);
                        pad = false;
                    }
                n[4] += pad;
                bool punt = false;
                order += run_entry(c, e2, pad, order, sink, punt);
                if (punt) return -34;
            }
            continue;
        }
        if (st != SPAN_OK) return -35;
        ++n[0];
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: loadsim <case file> <record file>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t h[6]; int64_t m[3];
    thj_params tp;
    if (fread(h, 4, 6, f) != 6 || fread(m, 8, 3, f) != 3 || fread(&tp, sizeof tp, 1, f) != 1 || h[0] != 0x4C4F4144) { fprintf(stderr, "loadsim: bad case file\n"); return 2; }
    Case c;
    static_assert(sizeof(Params) == sizeof(thj_params), "Params == thj_params");
    memcpy(&c.p, &tp, sizeof tp);
    const int32_t n_contigs = h[1];
    c.n_reads = h[2]; c.nseg = h[3]; c.W = h[4]; c.qual_stride = h[5]; c.n_hits = m[1];
    const u64* blocks = take<u64>(f, (size_t)m[0]);
    const uint32_t* contig_blk = take<uint32_t>(f, (size_t)n_contigs + 1);
    const int32_t* contig_len = take<int32_t>(f, (size_t)n_contigs);
    c.g = Genome{blocks, contig_blk, contig_len, n_contigs};
    c.seg_off = take<uint32_t>(f, (size_t)c.n_reads * c.nseg + 1);
    c.hits = take<SpanHit>(f, (size_t)m[1]);
    c.planes = take<u64>(f, (size_t)c.n_reads * 3 * c.W);
    c.read_len = take<uint16_t>(f, (size_t)c.n_reads);
    c.quals = take<uint8_t>(f, (size_t)c.n_reads * c.qual_stride);
    const thj_junction* juncs = take<thj_junction>(f, (size_t)m[2]);
    fclose(f);
    u64* jk = (u64*)malloc(m[2] ? m[2] * sizeof(u64) : 1);
    for (int64_t i = 0; i < m[2]; ++i) jk[i] = junc_key(c.g, juncs[i].ref_id, juncs[i].left, juncs[i].right, juncs[i].antisense != 0);
    for (int64_t i = 1; i < m[2]; ++i) if (jk[i] <= jk[i - 1]) { fprintf(stderr, "loadsim: junctions not sorted\n"); return 2; }
    c.S = SpanSets{jk, m[2], nullptr, nullptr, 0, nullptr, 0};
    std::vector<std::vector<OutAln>> outs((size_t)c.n_reads);
    long n[6] = {0, 0, 0, 0, 0, 0};
    const int rc = c.nseg <= 4 ? run<4>(c, outs, n) : c.nseg <= SPAN_MIDSEG ? run<SPAN_MIDSEG>(c, outs, n) : -36;
    if (rc) { fprintf(stderr, "loadsim: read outside the sim's paths (%d)\n", rc); return 3; }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    long n_rec = 0;
    for (auto& v : outs) for (auto& a : v) { fwrite(&a, sizeof a, 1, o); ++n_rec; }
    fclose(o);
    printf("LOADSIM tier0 %ld chain %ld lean %ld groups %ld padding %ld records %ld\n", n[0], n[1], n[2], n[3], n[4], n_rec);
    free((void*)blocks); free((void*)contig_blk); free((void*)contig_len); free((void*)c.seg_off); free((void*)c.hits); free((void*)c.planes);
    free((void*)c.read_len); free((void*)c.quals); free((void*)juncs); free(jk);
    return 0;
}
