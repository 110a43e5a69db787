// TEST-ONLY: the per-record and per-junction decisions of the junction consensus' two switches (tophat_amd/csrc/thj_jbknown_core.h:
// the read filter's three quantities and its verdict, the annotation lookup, accept, "is exempt from the knockout") and the
// --gtf-juncs line reader of thj_junctions (thj_hostio.h: load_gtf_juncs), compiled for the CPU.
//
//     jbknownsim consensus <cases.txt>
// one consensus per "E" line of the file; the lines before it:
//     A <min_anchor>
//     F <on> <read_mismatches> <read_gap_length> <read_edit_dist>
//     C <length of contig 1> <length of contig 2> ...
//     K <ref_id> <left> <right> <antisense>                       an entry of the annotation, as handed to thj_juncbed_known_junctions
//     R <ref_id> <left> <antisense> <NM, -1: no tag> <ref_id2> <n> <op> <len> ...     a record
// and what is printed for it:
//     R <mismatches> <gap_length> <dropped 0|1>                    per record, in order
//     J <ref_id> <left> <right> <antisense> <acc> <acc2>           per distinct junction of the records kept, in Junction::operator< order
//     O <ref_id> <left> <right> <antisense> <left_extent> <right_extent> <support>      the final set
//     E
// The two passes around the decisions are the plain loops of the reference (junctions.cpp:242-318, tophat_reports.cpp:1194-1229,
// :2974-2984); the kernels of thj_juncbed_impl.h do the same over a hash table.
//
//     jbknownsim gtf <file> <contig,contig,...>
// the contigs the run knows, ref_id 1, 2, ... in that order -> "G <ref_id> <left> <right> <antisense>" per junction load_gtf_juncs
// returns; its message goes to stderr, and a malformed line ends the program with status 1 as it ends thj_junctions.
#include <algorithm>
#include <cstdio>
#include <map>

#include "../../tophat_amd/csrc/host/thj_hostio.h"
#include "../../tophat_amd/csrc/thj_jbknown_core.h"

using namespace thjh;

struct Rec { uint32_t ref, ref2; int32_t left; bool anti; int64_t nm; std::vector<uint32_t> cig; };
struct Junc { uint32_t ref, left, right, anti; bool operator<(const Junc& o) const { return std::tie(ref, left, right, anti) < std::tie(o.ref, o.left, o.right, o.anti); } };
struct Stat { uint32_t le = 0, re = 0, n = 0, acc = 0; bool acc2 = false; };

// junc_key's layout with every contig 2^27 bases apart (thj_core.h: [global left + 1 : 34 | right - left : 29 | antisense : 1])
static jbk::key64 key_of(const Junc& j) {
    const jbk::key64 gpos = ((jbk::key64)j.ref << 27) + (jbk::key64)(int64_t)(int32_t)j.left + 1ull;
    return (gpos << 30) | ((jbk::key64)((j.right - j.left) & (uint32_t)jbk::SPAN_MASK) << 1) | (j.anti ? 1ull : 0ull);
}

static void run_case(int min_anchor, const jbk::ReadFilter& flt, const std::vector<int64_t>& lens, const std::vector<Junc>& annot, const std::vector<Rec>& recs) {
    std::vector<jbk::key64> known;
    for (auto& j : annot) if (jbk::known_entry_ok(j.ref, j.left, j.right, (int32_t)lens.size(), lens.data())) known.push_back(key_of(j));
    std::sort(known.begin(), known.end());
    known.erase(std::unique(known.begin(), known.end()), known.end());
    auto juncs_of = [](const Rec& r, std::vector<std::pair<Junc, std::pair<uint32_t, uint32_t>>>& out) {
        out.clear();
        jbw::juncs((int)r.cig.size(), r.left, r.ref, r.ref2, [&](int c) { return r.cig[(size_t)c]; }, [&](uint32_t ref, uint32_t l, uint32_t rt, uint32_t le, uint32_t re) {
            out.push_back({Junc{ref, l, rt, r.anti ? 1u : 0u}, {le, re}});
        });
    };
    std::vector<char> live(recs.size(), 1);
    std::vector<std::pair<Junc, std::pair<uint32_t, uint32_t>>> js;
    std::map<Junc, Stat> first;
    for (size_t i = 0; i < recs.size(); ++i) {
        const Rec& r = recs[i];
        auto cg = [&](int c) { return r.cig[(size_t)c]; };
        const uint8_t mism = jbk::mismatches(r.nm < 0 ? 0 : r.nm, (int)r.cig.size(), cg);
        const bool drop = flt.on && jbk::dropped(flt, mism, (int)r.cig.size(), cg);
        printf("R %u %u %d\n", (unsigned)mism, jbk::gap_length((int)r.cig.size(), cg), drop ? 1 : 0);
        live[i] = !drop;
        if (drop) continue;
        juncs_of(r, js);
        for (auto& j : js) { Stat& s = first[j.first]; s.le = std::max(s.le, j.second.first); s.re = std::max(s.re, j.second.second); ++s.n; }
    }
    for (auto& e : first) e.second.acc = jbk::accept(key_of(e.first), e.second.le, e.second.re, e.second.n, min_anchor, known.empty() ? nullptr : known.data(), (int64_t)known.size());
    for (auto& e : first) {                                     // knockout_shadow_junctions
        const Junc& k = e.first;
        bool ok = jbk::accepted(e.second.acc);
        if (ok && !jbk::exempt(e.second.acc) && k.left >= (uint32_t)min_anchor)
            for (auto& o : first) {
                const Junc& k2 = o.first;
                const Junc lo{k.ref, k.left - (uint32_t)min_anchor, k.right, 1u - k.anti}, hi{k.ref, k.left, k.right + (uint32_t)min_anchor, 1u - k.anti};
                if (&o == &e || k2.anti == k.anti || k2 < lo || hi < k2) continue;
                const int left_diff = (int)k.left - (int)k2.left, right_diff = (int)k.right - (int)k2.right;
                if ((left_diff < min_anchor || right_diff < min_anchor) && e.second.n < o.second.n) ok = false;
            }
        e.second.acc2 = ok;
        printf("J %u %u %u %u %u %d\n", k.ref, k.left, k.right, k.anti, e.second.acc, ok ? 1 : 0);
    }
    std::map<Junc, Stat> fin;
    for (size_t i = 0; i < recs.size(); ++i) {
        if (!live[i]) continue;
        juncs_of(recs[i], js);
        bool keep = true;
        for (auto& j : js) keep = keep && first[j.first].acc2;
        if (!keep) continue;
        for (auto& j : js) { Stat& s = fin[j.first]; s.le = std::max(s.le, j.second.first); s.re = std::max(s.re, j.second.second); ++s.n; }
    }
    for (auto& e : fin)
        if (e.second.n > 0 && e.second.le >= 8 && e.second.re >= 8) printf("O %u %u %u %u %u %u %u\n", e.first.ref, e.first.left, e.first.right, e.first.anti, e.second.le, e.second.re, e.second.n);
    printf("E\n");
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "gtf")) {
        RefTable rt;
        for (auto& n : split(argv[3], ',')) rt.get_id(n);
        rt.freeze();
        for (auto& j : load_gtf_juncs(argv[2], rt)) printf("G %u %u %u %u\n", j.ref_id, j.left, j.right, j.antisense);
        return 0;
    }
    if (argc != 3 || strcmp(argv[1], "consensus")) { fprintf(stderr, "usage: jbknownsim consensus <cases.txt> | jbknownsim gtf <file> <contig,contig,...>\n"); return 2; }
    FILE* f = fopen(argv[2], "r");
    if (!f) return 3;
    int min_anchor = 8;
    jbk::ReadFilter flt{};
    std::vector<int64_t> lens;
    std::vector<Junc> annot;
    std::vector<Rec> recs;
    char* line = nullptr; size_t cap = 0;
    while (getline(&line, &cap, f) > 0) {
        std::vector<long long> v;
        char* p = line + 1;
        for (;;) { char* e; const long long x = strtoll(p, &e, 10); if (e == p) break; v.push_back(x); p = e; }
        switch (line[0]) {
        case 'A': if (v.size() != 1) return 4; min_anchor = (int)v[0]; break;
        case 'F': if (v.size() != 4) return 4; flt = jbk::ReadFilter{(int32_t)v[0], (int32_t)v[1], (int32_t)v[2], (int32_t)v[3]}; break;
        case 'C': lens.assign(v.begin(), v.end()); break;
        case 'K': if (v.size() != 4) return 4; annot.push_back(Junc{(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], v[3] ? 1u : 0u}); break;
        case 'R': {
            if (v.size() < 6 || v.size() != 6 + 2 * (size_t)v[5] || v[5] > 16) return 4;
            Rec r{(uint32_t)v[0], (uint32_t)v[4], (int32_t)v[1], v[2] != 0, v[3], {}};
            for (size_t k = 6; k < v.size(); k += 2) r.cig.push_back((uint32_t)v[k] << 28 | ((uint32_t)v[k + 1] & jbw::LEN_MASK));
            recs.push_back(r);
            break; }
        case 'E': run_case(min_anchor, flt, lens, annot, recs); annot.clear(); recs.clear(); break;
        default: break;
        }
    }
    free(line);
    fclose(f);
    return 0;
}
