// TEST-ONLY: the paired paths of tophat_amd/csrc/thj_accepted_core.h (emit() with a Mate, tlen_of, mate_flag_bits, xs_strand) and of
// thj_pair_core.h (happy(), the running best's happy bit) compiled for the CPU, laid out as the kernels of thj_accepted_pair_impl.h lay an
// insert's records out.
//
//   acceptedpairsim rewrite FILE
//       C <library_type> <rg or -> <n_ref>       the settings
//       N <ref_id> <out tid> <name>              a contig
//       P <draw> <n> <happy>                     an insert that reports n pairs: best_hits in order, per pair an L line, then an R line
//       S <draw> <n> <side 1|2>                  a side that goes alone: its n reported alignments in `hits` order, as R lines
//       L|R <ref_id> <left> <right> <antisense> <score> <hex>     a record: what the grade kept of it, and the input record without block_size
//     prints per insert / side "L <loud flags> <text>" when anything is loud, else per record in output order "O <hex>"
//   acceptedpairsim funcs FILE      one answer per line:
//       H <anti1> <spliced1> <antisplice1> <anti2> <spliced2> <antisplice2> <too_far>    jbp::happy
//       T <left> <right> <partner left> <partner right>                                  acc::tlen_of
//       X <library_type> <antisense> <side>                                              acc::xs_strand
//       B <n> then n times <score> <fusion> <happy>                                      the happy bit jbp::step leaves with the best
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../tophat_amd/csrc/thj_accepted_core.h"
#include "../../tophat_amd/csrc/thj_pair_core.h"

struct Rec { uint32_t ref; int32_t left, right; uint32_t anti; int32_t score; std::vector<uint8_t> d; };

static std::vector<uint32_t> index_vector(const std::vector<uint32_t>& ref, const std::vector<int32_t>& left) {
    const size_t n = ref.size();
    if (n > acc::SORT_BY_COUNTING) return acc::sort_places(ref, left);
    std::vector<uint32_t> iv(n);
    for (size_t i = 0; i < n; ++i) {
        uint32_t place = 0;
        for (size_t j = 0; j < n; ++j) place += j != i && acc::lex_before(ref[j], left[j], (uint32_t)j, ref[i], left[i], (uint32_t)i);
        iv[place] = (uint32_t)i;
    }
    return iv;
}

static bool parse_rec(const char* s, Rec& r) {
    int used = 0;
    if (sscanf(s, "%u %d %d %u %d %n", &r.ref, &r.left, &r.right, &r.anti, &r.score, &used) < 5) return false;
    for (const char* q = s + used; q[0] && q[1] && q[0] != '\n'; q += 2) { unsigned b; sscanf(q, "%2x", &b); r.d.push_back((uint8_t)b); }
    return true;
}

// one record through both sinks; false: loud
static bool write_one(const Rec& r, const acc::Cfg& cfg, const acc::Slot& s, const acc::Mate& m, std::vector<uint8_t>& out, uint32_t& loud) {
    acc::NullSink cnt;
    uint32_t l1 = 0;
    const uint32_t size = acc::emit(r.d.data(), (uint32_t)r.d.size(), cfg, s, cnt, l1, m);
    loud |= l1;
    if (l1) return false;
    out.resize(size);
    acc::MemSink mem{out.data()};
    uint32_t l2 = 0;
    const uint32_t size2 = acc::emit(r.d.data(), (uint32_t)r.d.size(), cfg, s, mem, l2, m);
    if (size2 != size || l2) { fprintf(stderr, "ERROR: the two walks differ\n"); exit(3); }
    return true;
}

static acc::Mate mate_of(uint32_t side, const Rec* partner, bool happy) {
    acc::Mate m;
    m.side = side;
    if (partner) { m.partner = 1; m.ref_id = partner->ref; m.left = partner->left; m.right = partner->right; m.anti = partner->anti; m.happy = happy ? 1u : 0u; }
    return m;
}

static int funcs(FILE* f) {
    char line[1 << 16];
    while (fgets(line, sizeof line, f)) {
        if (line[0] == 'H') {
            unsigned a1, s1, x1, a2, s2, x2, tf;
            if (sscanf(line + 1, "%u %u %u %u %u %u %u", &a1, &s1, &x1, &a2, &s2, &x2, &tf) != 7) return 2;
            jbp::Hit h1{1, 0, 0, 0, (uint8_t)a1, 0, (uint8_t)s1, (uint8_t)x1}, h2{1, 0, 0, 0, (uint8_t)a2, 0, (uint8_t)s2, (uint8_t)x2};
            printf("%d\n", jbp::happy(h1, h2, tf != 0) ? 1 : 0);
        } else if (line[0] == 'T') {
            int l, r, pl, pr;
            if (sscanf(line + 1, "%d %d %d %d", &l, &r, &pl, &pr) != 4) return 2;
            printf("%d\n", acc::tlen_of(l, r, pl, pr));
        } else if (line[0] == 'X') {
            int lt; unsigned anti, side;
            if (sscanf(line + 1, "%d %u %u", &lt, &anti, &side) != 3) return 2;
            printf("%c\n", acc::xs_strand(lt, anti != 0, side));
        } else if (line[0] == 'B') {
            int n = 0, used = 0;
            if (sscanf(line + 1, "%d %n", &n, &used) < 1) return 2;
            const char* q = line + 1 + used;
            jbp::Cfg cfg{200, 20, 10000000, 6, 20, 0, 0, 0, 1};
            jbp::Running run{0, 0, 0, 0};
            for (int k = 0; k < n; ++k) {
                int sc, fu, hp, u2 = 0;
                if (sscanf(q, "%d %d %d %n", &sc, &fu, &hp, &u2) < 3) return 2;
                q += u2;
                (void)jbp::step(run, sc, fu != 0, cfg, hp != 0);
            }
            printf("%d\n", run.any ? (int)run.best_happy : -1);
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: acceptedpairsim rewrite|funcs FILE\n"); return 2; }
    FILE* f = fopen(argv[2], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    if (!strcmp(argv[1], "funcs")) { const int rc = funcs(f); fclose(f); if (rc) fprintf(stderr, "bad line\n"); return rc; }
    std::vector<char> line(1 << 20);
    acc::Cfg cfg{};
    acc::mapq_table(cfg.mapq);
    std::string rg, blob;
    std::vector<int32_t> tid_of_ref;
    std::vector<uint32_t> name_off{0};
    std::vector<Rec> ls, rs;
    unsigned long draw = 0; unsigned kind = 0, happy = 0, side = 0;      // kind 1: pairs, 2: a side alone
    auto hex_out = [](const std::vector<uint8_t>& v) { fputs("O ", stdout); for (uint8_t b : v) printf("%02x", b); putchar('\n'); };
    auto flush = [&]() {
        if (!kind || rs.empty()) { kind = 0; ls.clear(); rs.clear(); return; }
        cfg.rg = (const uint8_t*)rg.data(); cfg.rg_len = (uint32_t)rg.size();
        cfg.tid_of_ref = tid_of_ref.data(); cfg.n_ref = (int32_t)tid_of_ref.size();
        cfg.names = (const uint8_t*)blob.data(); cfg.name_off = name_off.data();
        const size_t n = rs.size();
        if (kind == 1 && ls.size() != n) { fprintf(stderr, "ERROR: an insert's L and R lines differ in number\n"); exit(2); }
        std::vector<uint32_t> ref(n); std::vector<int32_t> left(n);
        for (size_t i = 0; i < n; ++i) { ref[i] = rs[i].ref; left[i] = rs[i].left; }       // lex_hit_sort over the RIGHT records of best_hits / over a read's hits
        const std::vector<uint32_t> iv = index_vector(ref, left);
        const uint32_t primary = (uint32_t)(draw % n);
        std::vector<std::vector<uint8_t>> out;
        uint32_t loud = 0;
        for (size_t p = 0; p < n; ++p) {
            const uint32_t k = iv[p];
            for (int which = 0; which < (kind == 1 ? 2 : 1); ++which) {
                const std::vector<Rec>& mine = which ? ls : rs;
                const Rec& r = mine[k];
                acc::Slot s{};
                s.n = (uint32_t)n; s.place = (uint32_t)p; s.ref_id = r.ref; s.score = r.score;
                s.flags = (k == primary ? acc::SLOT_PRIMARY : 0u) | (p + 1 < n ? acc::SLOT_HAS_NEXT : 0u);
                if (p + 1 < n) { s.next_ref = mine[iv[p + 1]].ref; s.next_left = mine[iv[p + 1]].left; }
                const acc::Mate m = kind == 1 ? mate_of(which ? acc::SIDE_LEFT : acc::SIDE_RIGHT, which ? &rs[k] : &ls[k], happy != 0) : mate_of(side, nullptr, false);
                out.emplace_back();
                write_one(r, cfg, s, m, out.back(), loud);
            }
        }
        if (loud) printf("L %u %s\n", loud, acc::loud_text(loud, true));
        else for (auto& o : out) hex_out(o);
        kind = 0; ls.clear(); rs.clear();
    };
    while (fgets(line.data(), (int)line.size(), f)) {
        char* s = line.data();
        if (s[0] == 'C') {
            flush();
            char rgb[4096]; int lt = 0, nr = 0;
            if (sscanf(s + 1, "%d %4095s %d", &lt, rgb, &nr) != 3) { fprintf(stderr, "bad C line\n"); return 2; }
            cfg.library_type = lt; rg = strcmp(rgb, "-") ? rgb : "";
            tid_of_ref.assign((size_t)nr, -1); name_off.assign((size_t)nr + 1, 0); blob.clear();
        } else if (s[0] == 'N') {
            unsigned r; int tid; char nm[4096];
            if (sscanf(s + 1, "%u %d %4095s", &r, &tid, nm) != 3 || r < 1 || r > tid_of_ref.size() || name_off[r - 1] != blob.size()) { fprintf(stderr, "bad N line\n"); return 2; }
            tid_of_ref[r - 1] = tid; blob += nm; name_off[r] = (uint32_t)blob.size();
        } else if (s[0] == 'P') {
            flush();
            unsigned n;
            if (sscanf(s + 1, "%lu %u %u", &draw, &n, &happy) != 3) { fprintf(stderr, "bad P line\n"); return 2; }
            kind = 1;
        } else if (s[0] == 'S') {
            flush();
            unsigned n;
            if (sscanf(s + 1, "%lu %u %u", &draw, &n, &side) != 3 || side < 1 || side > 2) { fprintf(stderr, "bad S line\n"); return 2; }
            kind = 2;
        } else if (s[0] == 'L' || s[0] == 'R') {
            Rec r;
            if (!parse_rec(s + 1, r)) { fprintf(stderr, "bad record line\n"); return 2; }
            (s[0] == 'L' ? ls : rs).push_back(std::move(r));
        }
    }
    flush();
    fclose(f);
    return 0;
}
