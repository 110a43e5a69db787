// TEST-ONLY: the choice among an insert's alignments (tophat_amd/csrc/thj_pair_core.h: distances, the fusion test, the grade with its
// rescue, the sequential list, the sort, the cap's split and draws), compiled for the CPU.
//
//     pairsim order
// scores on stdin -> the order libstdc++'s std::sort gives a list of pairs with these scores under cmp_pair_alignment (jbp::sort_order:
// what the library's host part runs for a list of more than 16, and what tests/pair_ref.py calls instead of restating std::sort).
//
//     pairsim lists
// stdin, one run per "E" line; the lines before it:
//     C <mean> <sd> <fusion_min_dist> <max_penalty> <max_multihits> <report_mixed> <report_discordant> <suppress_hits> <final_report>
//     J <ref_id> <left> <right> <first-pass support>                         a junction of the set the grade searches
//     D <n>                                                                  the generator has drawn n times before this insert
//     P <ref l.left l.right l.score l.anti l.fused l.eq> <the same of r>     a candidate, in generation order; eq: its cmp_read_equal class
// and what is printed:
//     G <allowed 0|1> <fusion 0|1> <score>                                   per candidate
//     L <candidate> ...                                                      the list after sort, unique and cap, by candidate number
//     S <best grade is a fusion grade 0|1> <over the cap 0|1> <draws used by the cap>
//     E
// The loops around the core's decisions are the plain ones of the reference, over the steps the kernels of thj_juncbed_pair_impl.h take:
// places by counting up to 16 entries, the host's std::sort beyond, neighbours for std::unique, better + ties for the cap.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../tophat_amd/csrc/thj_pair_core.h"

struct Junc { uint32_t ref; int left, right; uint32_t support; };
struct Cand { jbp::Hit l, r; int leq, req; };

static int run_order() {
    std::vector<int32_t> sc;
    long v;
    while (scanf("%ld", &v) == 1) sc.push_back((int32_t)v);
    std::vector<uint32_t> ord(sc.size());
    jbp::sort_order(sc.data(), (uint32_t)sc.size(), ord.data());
    for (size_t k = 0; k < ord.size(); ++k) printf("%s%u", k ? " " : "", ord[k]);
    printf("\n");
    return 0;
}

static void run_insert(const jbp::Cfg& cfg, const std::vector<Junc>& juncs, const std::vector<Cand>& cands, unsigned long long drawn) {
    struct Kept { int32_t score; uint32_t cand; };
    std::vector<Kept> kept;
    jbp::Running run{0, 0, 0};
    for (size_t k = 0; k < cands.size(); ++k) {
        const Cand& c = cands[k];
        if (!jbp::allowed(c.l, c.r)) { printf("G 0 0 0\n"); continue; }
        const bool fusion = jbp::is_fusion(c.l, c.r, cfg.fusion_min_dist);
        const int sc = jbp::grade(c.l, c.r, cfg, fusion, [&](uint32_t ref, int inner1, int inner2) {
            for (const Junc& j : juncs) if (j.ref == ref && jbp::rescues(j.left, j.right, j.support, inner1, inner2, cfg)) return true;
            return false;
        });
        printf("G 1 %d %d\n", fusion ? 1 : 0, sc);
        const int act = jbp::step(run, sc, fusion, cfg);
        if (act == jbp::STEP_CLEAR_ENTER) kept.clear();
        if (act != jbp::STEP_SKIP) kept.push_back(Kept{sc, (uint32_t)k});
    }
    const uint32_t nk = (uint32_t)kept.size();
    std::vector<uint32_t> order(nk);
    if (nk <= jbp::SORT_SMALL) for (uint32_t a = 0; a < nk; ++a) order[jbp::place16(nk, a, [&](uint32_t k) { return kept[k].score; })] = a;
    else { std::vector<int32_t> sc(nk); for (uint32_t k = 0; k < nk; ++k) sc[k] = kept[k].score; jbp::sort_order(sc.data(), nk, order.data()); }
    std::vector<Kept> left;
    for (uint32_t p = 0; p < nk; ++p) {
        const Kept& k = kept[order[p]];
        if (!left.empty() && cands[left.back().cand].leq == cands[k.cand].leq && cands[left.back().cand].req == cands[k.cand].req) continue;
        left.push_back(k);
    }
    bool over = false;
    unsigned long long used = 0;
    if (cfg.final_report) {
        over = left.size() > (size_t)cfg.max_multihits;
        if (over && cfg.suppress) left.clear();
        if (left.size() > (size_t)cfg.max_multihits) {
            uint32_t better, ties;
            jbp::cap_split((uint32_t)left.size(), (uint32_t)cfg.max_multihits, [&](uint32_t k) { return left[k].score; }, better, ties);
            jbb::Mt19937 rng;
            rng.seed(1u);
            rng.discard(drawn);
            std::vector<uint8_t> alive(ties, 1);
            jbp::trim_pairs(better, ties, (uint32_t)cfg.max_multihits, [&]() { ++used; return rng.next(); }, alive.data());
            std::vector<Kept> out(left.begin(), left.begin() + better);
            for (uint32_t k = 0; k < ties; ++k) if (alive[k]) out.push_back(left[better + k]);
            left.swap(out);
        }
    }
    printf("L");
    for (const Kept& k : left) printf(" %u", k.cand);
    printf("\nS %d %d %llu\nE\n", run.best_fusion ? 1 : 0, over ? 1 : 0, used);
}

static int run_lists() {
    jbp::Cfg cfg{200, 20, 10000000, 6, 20, 0, 0, 0, 1};
    std::vector<Junc> juncs;
    std::vector<Cand> cands;
    unsigned long long drawn = 0;
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        if (line[0] == 'C') {
            int v[9];
            if (sscanf(line + 1, "%d %d %d %d %d %d %d %d %d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8) != 9 || v[1] < 1 || v[4] < 1) { fprintf(stderr, "bad C line\n"); return 2; }
            cfg = jbp::Cfg{v[0], v[1], v[2], v[3], v[4], (uint8_t)v[5], (uint8_t)v[6], (uint8_t)v[7], (uint8_t)v[8]};
        } else if (line[0] == 'J') {
            Junc j;
            if (sscanf(line + 1, "%u %d %d %u", &j.ref, &j.left, &j.right, &j.support) != 4) { fprintf(stderr, "bad J line\n"); return 2; }
            juncs.push_back(j);
        } else if (line[0] == 'D') {
            if (sscanf(line + 1, "%llu", &drawn) != 1) { fprintf(stderr, "bad D line\n"); return 2; }
        } else if (line[0] == 'P') {
            Cand c;
            int la, lf, ra, rf;
            if (sscanf(line + 1, "%u %d %d %d %d %d %d %u %d %d %d %d %d %d", &c.l.ref_id, &c.l.left, &c.l.right, &c.l.score, &la, &lf, &c.leq, &c.r.ref_id, &c.r.left, &c.r.right,
                       &c.r.score, &ra, &rf, &c.req) != 14) { fprintf(stderr, "bad P line\n"); return 2; }
            c.l.anti = (uint8_t)la; c.l.fused = (uint8_t)lf; c.r.anti = (uint8_t)ra; c.r.fused = (uint8_t)rf;
            cands.push_back(c);
        } else if (line[0] == 'E') {
            run_insert(cfg, juncs, cands, drawn);
            juncs.clear(); cands.clear(); drawn = 0;
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "order")) return run_order();
    if (argc == 2 && !strcmp(argv[1], "lists")) return run_lists();
    fprintf(stderr, "usage: pairsim order | pairsim lists   (input on stdin)\n");
    return 2;
}
