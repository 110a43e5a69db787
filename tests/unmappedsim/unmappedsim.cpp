// TEST-ONLY: tophat_amd/csrc/thj_unmapped_core.h compiled for the CPU -- the decisions and the record of thj_juncbed_report_unmapped_bam as the
// kernels of thj_unmapped.hip run them: a record of a reads file is parsed, its number looked up among the groups by binary search, decided,
// counted and written through the plain-memory sink.
//
//   unmappedsim run FILE
//       C <paired> <mixed>                      the run
//       G <number> <word> <code left> <code right>     a read with a group (single-end: word 0, its code first) or an insert, in rising number
//       I <number> <the thirteen arguments of `word`> <code left> <code right>     an insert whose word um::insert_word makes here
//       S <side>                                a reads file begins (0 left or only, 1 right)
//       R <hex>                                 one of its records, without the block_size field
//     prints per written record "O <side> <hex>", at the first loud record "L <flags> <text>" and stops, else at the end "T" and the
//     fifteen counters, then "F <left groups met> <right groups met>"
//   unmappedsim word <has_l> <has_r> <live_l> <live_r> <gone_l> <gone_r> <n_list> <best_fusion> <best_conc> <max_multihits> <suppress> <mixed> <discordant>
//   unmappedsim code <n> <max_multihits> <suppress>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../tophat_amd/csrc/thj_unmapped_core.h"

struct Group { uint64_t number; uint32_t word, code[2]; };

static int hexval(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

int main(int argc, char** argv) {
    if (argc == 15 && !strcmp(argv[1], "word")) {
        int v[13];
        for (int k = 0; k < 13; ++k) v[k] = atoi(argv[2 + k]);
        printf("%u\n", um::insert_word(v[0], v[1], v[2], v[3], v[4], v[5], (uint32_t)v[6], v[7], v[8], (uint32_t)v[9], v[10], v[11], v[12]));
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "code")) { printf("%u\n", um::read_code((uint32_t)atoi(argv[2]), (uint32_t)atoi(argv[3]), atoi(argv[4]) != 0)); return 0; }
    if (argc != 3 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: unmappedsim run FILE | word ... | code ...\n"); return 2; }
    FILE* f = fopen(argv[2], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    std::vector<char> line(1 << 20);
    um::Run run{0, 0};
    std::vector<Group> groups;
    long long stats[um::N_STATS] = {0}, met[2] = {0, 0};
    uint32_t side = 0;
    uint64_t prev = 0;
    while (fgets(line.data(), (int)line.size(), f)) {
        const char* s = line.data();
        if (s[0] == 'C') { int p, m; if (sscanf(s + 1, "%d %d", &p, &m) != 2) return 2; run.paired = (uint8_t)p; run.mixed = (uint8_t)m; }
        else if (s[0] == 'G') { Group g; unsigned long long num; if (sscanf(s + 1, "%llu %u %u %u", &num, &g.word, &g.code[0], &g.code[1]) != 4) return 2; g.number = num; groups.push_back(g); }
        else if (s[0] == 'I') {
            Group g; unsigned long long num; int v[13];
            if (sscanf(s + 1, "%llu %d %d %d %d %d %d %d %d %d %d %d %d %d %u %u", &num, &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], &v[8], &v[9], &v[10], &v[11], &v[12],
                       &g.code[0], &g.code[1]) != 16) return 2;
            g.number = num; g.word = um::insert_word(v[0], v[1], v[2], v[3], v[4], v[5], (uint32_t)v[6], v[7], v[8], (uint32_t)v[9], v[10], v[11], v[12]);
            groups.push_back(g);
        }
        else if (s[0] == 'S') { side = (uint32_t)atoi(s + 1); prev = 0; }
        else if (s[0] == 'R') {
            std::vector<uint8_t> rec;
            for (const char* p = s + 2; hexval(p[0]) >= 0 && hexval(p[1]) >= 0; p += 2) rec.push_back((uint8_t)(hexval(p[0]) * 16 + hexval(p[1])));
            um::Read r;
            um::parse(rec.data(), (uint32_t)rec.size(), r);
            uint32_t loud = r.loud;
            if (!loud && r.number <= prev) loud = um::LOUD_ORDER;
            um::Decision d{0, 0, 0};
            if (!loud) {
                prev = r.number;
                size_t a = 0, b = groups.size();
                while (a < b) { const size_t m = (a + b) >> 1; if (groups[m].number < r.number) a = m + 1; else b = m; }
                const bool found = a < groups.size() && groups[a].number == r.number;
                const uint32_t word = found && run.paired ? groups[a].word : 0u, code = found ? groups[a].code[run.paired ? side : 0] : 0u;
                if (found && (!run.paired || (word & (side ? um::W_HAS_R : um::W_HAS_L)))) ++met[side];
                d = um::decide(run, side, found, word, code, r.zt, r.matenum);
                loud = d.loud;
            }
            if (loud) { printf("L %u %s\n", loud, um::loud_text(loud)); fclose(f); return 0; }
            for (int k = 0; k < um::N_STATS; ++k) stats[k] += (d.counters >> k) & 1u;
            if (d.write) {
                std::vector<uint8_t> o(um::record_size(r));     // exactly the size the counting pass gives: the sanitizer sees a byte too many
                um::MemSink sink;
                sink.o = o.data();
                const uint32_t n = um::emit(rec.data(), r, sink);
                if (n != o.size()) { fprintf(stderr, "emit wrote %u bytes, record_size says %zu\n", n, o.size()); return 3; }
                um::NullSink cnt;
                if (um::emit(rec.data(), r, cnt) != n) { fprintf(stderr, "the counting sink disagrees\n"); return 3; }
                printf("O %u ", side);
                for (uint8_t x : o) printf("%02x", x);
                putchar('\n');
            }
        }
    }
    fclose(f);
    printf("T");
    for (int k = 0; k < um::N_STATS; ++k) printf(" %lld", stats[k]);
    printf("\nF %lld %lld\n", met[0], met[1]);
    return 0;
}
