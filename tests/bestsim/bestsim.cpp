// TEST-ONLY: the choice among a read's alignments (tophat_amd/csrc/thj_best_core.h: order, equality, score walk, penalty, the cap's
// trimming, the generator) and the AS:i parse of the record core (thj_reported_core.h), compiled for the CPU.
//
//     bestsim mt
// the first 1000 outputs of jbb::Mt19937 seeded 1 against std::mt19937 seeded 1 -> "MT ok <first four outputs>" or status 1.
//
//     bestsim choose <cases.txt>
// one run per "E" line; the lines before it:
//     A <min_anchor>
//     F <on> <read_mismatches> <read_gap_length> <read_edit_dist>
//     C <length of contig 1> <length of contig 2> ...
//     B <max_multihits> <suppress_hits> <bowtie2_max_penalty>
//     K <ref_id> <left> <right> <antisense>                       an entry of the annotation
//     R <read> <AS> <antisense_align> <mismatches> <ref_id> <left> <antisense_splice> <ref_id2> <n> <op> <len> ...     a record
// and what is printed:
//     R <rank, -1: dropped by the filter> <pass-1 duplicate 0|1> <score, x: it does not compete> <keep 0|1>        per record, in order
//     W <first record of a read over the cap> <number of its first draw in the stream> <surviving places ...>     per such read, in order
//     S <reads> <reads that lost records to the choice> <reads over the cap> <pass-1 duplicates>
//     E
// The loops around the core's decisions are the plain ones of the reference, over the steps the kernels of thj_juncbed_best_impl.h
// take: rank by counting the records below, the record just below for std::unique, a junction only duplicates show has support 0.
//
//     bestsim as <in.bam>
// rpt::reported_record with best alignments chosen over every record -> "K <AS>" or "D <report bits>".
#include <algorithm>
#include <cstdio>
#include <map>
#include <random>

#include "../../tophat_amd/csrc/host/thj_hostio.h"
#include "../../tophat_amd/csrc/thj_best_core.h"
#include "../../tophat_amd/csrc/thj_reported_core.h"

using namespace thjh;

struct Rec { uint32_t read; int AS; bool anti_aln; uint32_t mism, ref; int32_t left; bool anti; uint32_t cig[16]; int n; };
struct Junc { uint32_t ref, left, right, anti; bool operator<(const Junc& o) const { return std::tie(ref, left, right, anti) < std::tie(o.ref, o.left, o.right, o.anti); } };
struct Stat { uint32_t le = 0, re = 0, n = 0, acc = 0; bool acc2 = false; };
struct Cfg { int min_anchor = 8; jbk::ReadFilter flt{}; std::vector<int64_t> lens; uint32_t max_multihits = 20; bool suppress = false; int max_penalty = 6; };

static jbk::key64 key_of(const Junc& j) {                       // junc_key's layout with every contig 2^27 bases apart
    const jbk::key64 gpos = ((jbk::key64)j.ref << 27) + (jbk::key64)(int64_t)(int32_t)j.left + 1ull;
    return (gpos << 30) | ((jbk::key64)((j.right - j.left) & (uint32_t)jbk::SPAN_MASK) << 1) | (j.anti ? 1ull : 0ull);
}

static void run_case(const Cfg& cf, const std::vector<Junc>& annot, const std::vector<Rec>& recs) {
    const size_t n = recs.size();
    std::vector<jbk::key64> known;
    for (auto& j : annot) if (jbk::known_entry_ok(j.ref, j.left, j.right, (int32_t)cf.lens.size(), cf.lens.data())) known.push_back(key_of(j));
    std::sort(known.begin(), known.end());
    known.erase(std::unique(known.begin(), known.end()), known.end());
    auto cg = [&](size_t i) { return jbw::ArrayCigar{recs[i].cig}; };
    std::vector<char> live(n), dup(n, 0), keep(n, 0), scored(n, 0);
    std::vector<int> rank(n, -1), score(n, 0);
    std::vector<jbb::Key> key(n);
    for (size_t i = 0; i < n; ++i) {
        const Rec& r = recs[i];
        live[i] = !(cf.flt.on && jbk::dropped(cf.flt, r.mism, r.n, cg(i)));
        key[i] = jbb::key_of(r.ref, r.left, r.anti_aln, r.mism, r.n, cg(i));
    }
    std::vector<std::pair<size_t, size_t>> reads;
    for (size_t s = 0, i = 1; i <= n; ++i) if (i == n || recs[i].read != recs[s].read) { reads.push_back({s, i}); s = i; }
    auto below = [&](size_t j, size_t i) { return jbb::less(key[j], cg(j), key[i], cg(i)) || (j < i && !jbb::less(key[i], cg(i), key[j], cg(j))); };
    size_t n_dup = 0;
    for (auto& rd : reads)
        for (size_t i = rd.first; i < rd.second; ++i) {
            if (!live[i]) continue;
            int rk = 0; long pred = -1;
            for (size_t j = rd.first; j < rd.second; ++j) {
                if (j == i || !live[j] || !below(j, i)) continue;
                ++rk;
                if (pred < 0 || below((size_t)pred, j)) pred = (long)j;
            }
            rank[i] = rk;
            dup[i] = pred >= 0 && jbb::equal(key[(size_t)pred], key[i]);
            n_dup += dup[i];
        }
    // the first pass: a duplicate's junctions are in the table, with nothing added
    std::vector<std::vector<std::pair<Junc, std::pair<uint32_t, uint32_t>>>> js(n);
    std::map<Junc, Stat> first;
    for (size_t i = 0; i < n; ++i) {
        if (!live[i]) continue;
        const Rec& r = recs[i];
        jbw::juncs(r.cig, r.n, r.left, r.ref, [&](uint32_t ref, uint32_t l, uint32_t rt, uint32_t le, uint32_t re) { js[i].push_back({Junc{ref, l, rt, r.anti ? 1u : 0u}, {le, re}}); });
        for (auto& j : js[i]) { Stat& s = first[j.first]; if (dup[i]) continue; s.le = std::max(s.le, j.second.first); s.re = std::max(s.re, j.second.second); ++s.n; }
    }
    for (auto& e : first) {
        e.second.acc = jbk::accept(key_of(e.first), e.second.le, e.second.re, e.second.n, cf.min_anchor, known.empty() ? nullptr : known.data(), (int64_t)known.size());
        if (e.second.n == 0 && e.second.acc != jbk::ACC_KNOWN) e.second.acc = jbk::ACC_REJECTED;
    }
    for (auto& e : first) {                                     // knockout_shadow_junctions
        const Junc& k = e.first;
        bool ok = jbk::accepted(e.second.acc);
        if (ok && !jbk::exempt(e.second.acc) && k.left >= (uint32_t)cf.min_anchor)
            for (auto& o : first) {
                const Junc& k2 = o.first;
                const Junc lo{k.ref, k.left - (uint32_t)cf.min_anchor, k.right, 1u - k.anti}, hi{k.ref, k.left, k.right + (uint32_t)cf.min_anchor, 1u - k.anti};
                if (&o == &e || k2.anti == k.anti || k2 < lo || hi < k2) continue;
                const int left_diff = (int)k.left - (int)k2.left, right_diff = (int)k.right - (int)k2.right;
                if ((left_diff < cf.min_anchor || right_diff < cf.min_anchor) && e.second.n < o.second.n) ok = false;
            }
        e.second.acc2 = ok;
    }
    // the second pass
    for (size_t i = 0; i < n; ++i) {
        if (!live[i]) continue;
        bool ok = true;
        for (auto& j : js[i]) ok = ok && first[j.first].acc2;
        if (!ok) continue;
        const Rec& r = recs[i];
        scored[i] = 1;
        score[i] = jbb::score(r.AS, r.n, r.left, cf.max_penalty, cg(i), [&](int, uint32_t l, uint32_t rt) {
            jbb::Seen s{false, false, 0u, 0u, 0u};
            const Junc j{r.ref, l, rt, r.anti ? 1u : 0u};
            if (!jbk::known_entry_ok(j.ref, j.left, j.right, (int32_t)cf.lens.size(), cf.lens.data())) return s;      // it lies outside its contig: in no set
            s.annotated = !known.empty() && jbk::known(known.data(), (int64_t)known.size(), key_of(j));
            const auto it = first.find(j);
            if (!s.annotated && it != first.end() && it->second.n > 0) { s.found = true; s.support = it->second.n; s.left_extent = it->second.le; s.right_extent = it->second.re; }
            return s;
        });
    }
    size_t n_lost = 0, n_over = 0;
    unsigned long long stream = 0, since = 0;                   // draws so far; reporting reads since the last read over the cap
    jbb::CapWalk walk; walk.begin();
    std::vector<std::string> wlines;
    for (auto& rd : reads) {
        bool any = false; int best = 0;
        for (size_t i = rd.first; i < rd.second; ++i) if (scored[i] && (!any || score[i] > best)) { any = true; best = score[i]; }
        std::vector<size_t> left;
        bool lost = false;
        for (size_t i = rd.first; i < rd.second; ++i) {
            if (!live[i]) continue;
            bool kp = scored[i] && score[i] == best;
            if (kp) {
                long pred = -1;
                for (size_t j = rd.first; j < rd.second; ++j)
                    if (j != i && scored[j] && score[j] == best && rank[j] < rank[i] && (pred < 0 || rank[j] > rank[(size_t)pred])) pred = (long)j;
                kp = !(pred >= 0 && jbb::equal(key[(size_t)pred], key[i]));
            }
            if (kp) left.push_back(i); else lost = true;
        }
        n_lost += lost;
        std::sort(left.begin(), left.end(), [&](size_t a, size_t b) { return rank[a] < rank[b]; });
        if (left.size() > cf.max_multihits) {
            ++n_over;
            if (cf.suppress) left.clear();
            else {
                std::vector<uint8_t> alive(left.size(), 1);
                walk.read(since, (uint32_t)left.size(), cf.max_multihits, alive.data());
                std::string w = "W " + std::to_string(rd.first) + " " + std::to_string(stream + since);
                std::vector<size_t> surv;
                for (size_t k = 0; k < left.size(); ++k) if (alive[k]) { surv.push_back(left[k]); w += " " + std::to_string(k); }
                stream += since + (left.size() - cf.max_multihits) + 1; since = 0;
                left = surv;
                wlines.push_back(w);
                for (size_t i : left) keep[i] = 1;
                continue;
            }
        }
        if (!left.empty()) ++since;
        for (size_t i : left) keep[i] = 1;
    }
    for (size_t i = 0; i < n; ++i) {
        printf("R %d %d ", rank[i], dup[i] ? 1 : 0);
        if (scored[i]) printf("%d", score[i]); else printf("x");
        printf(" %d\n", keep[i] ? 1 : 0);
    }
    for (auto& w : wlines) printf("%s\n", w.c_str());
    printf("S %zu %zu %zu %zu\nE\n", reads.size(), n_lost, n_over, n_dup);
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "mt")) {
        jbb::Mt19937 g; g.seed(1u);
        std::mt19937 ref(1u);
        uint32_t head[4] = {0, 0, 0, 0};
        for (int i = 0; i < 1000; ++i) { const uint32_t x = g.next(); if (i < 4) head[i] = x; if (x != (uint32_t)ref()) { printf("MT differs at %d\n", i); return 1; } }
        printf("MT ok %u %u %u %u\n", head[0], head[1], head[2], head[3]);
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "as")) {
        AlnReader rd;
        if (!rd.open(argv[2]) || !rd.is_bam()) return 3;
        std::vector<uint32_t> tid2ref;
        for (size_t t = 0; t < rd.targets().size(); ++t) tid2ref.push_back((uint32_t)t + 1u);
        const uint8_t none = 0; const uint32_t zero = 0;
        rpt::Cfg cfg;
        cfg.tid2ref = tid2ref.data(); cfg.n_tid = (uint32_t)tid2ref.size(); cfg.max_report_intron = 500000; cfg.indels = false; cfg.fusions = true; cfg.best = true;
        cfg.names = rpt::Names{&none, &zero, &zero, 0};
        int32_t bs = 0;
        while (const uint8_t* d = rd.next_raw(bs)) {
            std::vector<uint8_t> rec(d, d + bs);                // the record on its own, so that a sanitizer sees a read past its end
            thj_aln a; memset(&a, 0xEE, sizeof a);
            rpt::Seq s; uint32_t n_ins = 0, rep = 0;
            if (rpt::reported_record(rec.data(), (uint32_t)bs, cfg, a, s, n_ins, rep)) printf("K %d\n", (int)a.AS); else printf("D %u\n", rep);
        }
        return 0;
    }
    if (argc != 3 || strcmp(argv[1], "choose")) { fprintf(stderr, "usage: bestsim mt | bestsim choose <cases.txt> | bestsim as <in.bam>\n"); return 2; }
    FILE* f = fopen(argv[2], "r");
    if (!f) return 3;
    Cfg cf;
    std::vector<Junc> annot;
    std::vector<Rec> recs;
    char* line = nullptr; size_t cap = 0;
    while (getline(&line, &cap, f) > 0) {
        std::vector<long long> v;
        char* p = line + 1;
        for (;;) { char* e; const long long x = strtoll(p, &e, 10); if (e == p) break; v.push_back(x); p = e; }
        switch (line[0]) {
        case 'A': if (v.size() != 1) return 4; cf.min_anchor = (int)v[0]; break;
        case 'F': if (v.size() != 4) return 4; cf.flt = jbk::ReadFilter{(int32_t)v[0], (int32_t)v[1], (int32_t)v[2], (int32_t)v[3]}; break;
        case 'C': cf.lens.assign(v.begin(), v.end()); break;
        case 'B': if (v.size() != 3 || v[0] < 1) return 4; cf.max_multihits = (uint32_t)v[0]; cf.suppress = v[1] != 0; cf.max_penalty = (int)v[2]; break;
        case 'K': if (v.size() != 4) return 4; annot.push_back(Junc{(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], v[3] ? 1u : 0u}); break;
        case 'R': {
            if (v.size() < 9 || v.size() != 9 + 2 * (size_t)v[8] || v[8] > 16 || (v[7] && v[8] > 15)) return 4;
            Rec r{(uint32_t)v[0], (int)v[1], v[2] != 0, (uint32_t)v[3], (uint32_t)v[4], (int32_t)v[5], v[6] != 0, {}, (int)v[8]};
            for (size_t k = 9, c = 0; k < v.size(); k += 2, ++c) r.cig[c] = (uint32_t)v[k] << 28 | ((uint32_t)v[k + 1] & jbw::LEN_MASK);
            r.cig[15] = v[7] ? (uint32_t)v[7] : r.cig[15];
            recs.push_back(r);
            break; }
        case 'E': run_case(cf, annot, recs); annot.clear(); recs.clear(); break;
        default: break;
        }
    }
    free(line);
    fclose(f);
    return 0;
}
