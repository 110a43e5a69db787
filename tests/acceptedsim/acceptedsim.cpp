// TEST-ONLY: tophat_amd/csrc/thj_accepted_core.h compiled for the CPU -- the record rewrite of thj_junctions --accepted-hits-out, the
// index_vector order and the MAPQ table, as the kernels of thj_accepted.hip and the host part of thj_juncbed_report_bam run them.
//
//   acceptedsim rewrite FILE    reads of planted records -> the rewritten records
//       C <library_type> <rg or -> <n_ref>       the settings
//       N <ref_id> <out tid> <name>              a contig
//       H <draw> <n>                             a read: the generator's raw output for it, its n reported alignments in `hits` order
//       R <ref_id> <score> <hex>                 one of them: contig, AlignStatus score, the input record without its block_size field
//     prints per read "L <loud flags> <text>" when anything is loud, else per record in index_vector order "O <hex>"
//   acceptedsim order FILE      lines "<ref_id> <left>" in `hits` order -> index_vector, one line (counting up to 16, std::sort beyond)
//   acceptedsim mapq            the table
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../tophat_amd/csrc/thj_accepted_core.h"

struct Hit { uint32_t ref; int32_t score; std::vector<uint8_t> rec; };

// index_vector: by counting for at most 16 entries (what the kernels do), std::sort itself beyond
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

static void hex_out(const char* tag, const std::vector<uint8_t>& v) {
    fputs(tag, stdout);
    for (uint8_t b : v) printf("%02x", b);
    putchar('\n');
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "mapq")) {
        uint8_t t[8];
        acc::mapq_table(t);
        printf("MAPQ %d %d %d %d %d %d\n", t[1], t[2], t[3], t[4], t[5], t[6]);
        return 0;
    }
    if (argc < 3) { fprintf(stderr, "usage: acceptedsim rewrite|order FILE | mapq\n"); return 2; }
    FILE* f = fopen(argv[2], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    std::vector<char> line(1 << 20);
    if (!strcmp(argv[1], "order")) {
        std::vector<uint32_t> ref; std::vector<int32_t> left;
        unsigned r; int l;
        while (fscanf(f, "%u %d", &r, &l) == 2) { ref.push_back(r); left.push_back(l); }
        const std::vector<uint32_t> iv = index_vector(ref, left);
        for (size_t i = 0; i < iv.size(); ++i) printf(i ? " %u" : "%u", iv[i]);
        putchar('\n');
        fclose(f);
        return 0;
    }
    acc::Cfg cfg{};
    acc::mapq_table(cfg.mapq);
    std::string rg, blob;
    std::vector<int32_t> tid_of_ref;
    std::vector<uint32_t> name_off{0};
    std::vector<Hit> hits;
    unsigned long draw = 0; size_t want = 0;
    auto flush = [&]() {
        if (hits.empty()) return;
        cfg.rg = (const uint8_t*)rg.data(); cfg.rg_len = (uint32_t)rg.size();
        cfg.tid_of_ref = tid_of_ref.data(); cfg.n_ref = (int32_t)tid_of_ref.size();
        cfg.names = (const uint8_t*)blob.data(); cfg.name_off = name_off.data();
        const size_t n = hits.size();
        std::vector<uint32_t> ref(n); std::vector<int32_t> left(n);
        for (size_t i = 0; i < n; ++i) { ref[i] = hits[i].ref; left[i] = hits[i].rec.size() >= 8 ? (int32_t)acc::rd32(hits[i].rec.data() + 4) : 0; }
        const std::vector<uint32_t> iv = index_vector(ref, left);
        const uint32_t primary = (uint32_t)(draw % n);
        std::vector<std::vector<uint8_t>> out(n);
        uint32_t loud = 0;
        for (size_t p = 0; p < n; ++p) {
            const Hit& h = hits[iv[p]];
            acc::Slot s{};
            s.n = (uint32_t)n; s.place = (uint32_t)p; s.ref_id = h.ref; s.score = h.score;
            s.flags = (iv[p] == primary ? acc::SLOT_PRIMARY : 0u) | (p + 1 < n ? acc::SLOT_HAS_NEXT : 0u);
            if (p + 1 < n) { s.next_ref = ref[iv[p + 1]]; s.next_left = left[iv[p + 1]]; }
            // first the size (the sink that only counts), then the bytes into exactly that much memory
            acc::NullSink cnt;
            uint32_t l1 = 0;
            const uint32_t size = acc::emit(h.rec.data(), (uint32_t)h.rec.size(), cfg, s, cnt, l1);
            loud |= l1;
            if (l1) continue;
            out[p].resize(size);
            acc::MemSink mem{out[p].data()};
            uint32_t l2 = 0;
            const uint32_t size2 = acc::emit(h.rec.data(), (uint32_t)h.rec.size(), cfg, s, mem, l2);
            if (size2 != size || l2) { fprintf(stderr, "ERROR: the two walks differ\n"); exit(3); }
        }
        if (loud) printf("L %u %s\n", loud, acc::loud_text(loud));
        else for (auto& o : out) hex_out("O ", o);
        hits.clear();
    };
    while (fgets(line.data(), (int)line.size(), f)) {
        char* s = line.data();
        if (s[0] == 'C') {
            flush();                                            // (the read before belongs to the settings before)
            char rgb[4096]; int lt = 0, nr = 0;
            if (sscanf(s + 1, "%d %4095s %d", &lt, rgb, &nr) != 3) { fprintf(stderr, "bad C line\n"); return 2; }
            cfg.library_type = lt; rg = strcmp(rgb, "-") ? rgb : "";
            tid_of_ref.assign((size_t)nr, -1); name_off.assign((size_t)nr + 1, 0); blob.clear();
        } else if (s[0] == 'N') {
            unsigned r; int tid; char nm[4096];
            if (sscanf(s + 1, "%u %d %4095s", &r, &tid, nm) != 3 || r < 1 || r > tid_of_ref.size() || name_off[r - 1] != blob.size()) { fprintf(stderr, "bad N line\n"); return 2; }
            tid_of_ref[r - 1] = tid; blob += nm; name_off[r] = (uint32_t)blob.size();
        } else if (s[0] == 'H') {
            flush();
            if (sscanf(s + 1, "%lu %zu", &draw, &want) != 2) { fprintf(stderr, "bad H line\n"); return 2; }
        } else if (s[0] == 'R') {
            Hit h; int used = 0;
            if (sscanf(s + 1, "%u %d %n", &h.ref, &h.score, &used) < 2) { fprintf(stderr, "bad R line\n"); return 2; }
            for (const char* q = s + 1 + used; q[0] && q[1] && q[0] != '\n'; q += 2) { unsigned b; sscanf(q, "%2x", &b); h.rec.push_back((uint8_t)b); }
            hits.push_back(std::move(h));
        }
    }
    flush();
    fclose(f);
    return 0;
}
