// TEST-ONLY: the spliced hit factory of the device-side ingest WITH its fusion branch (tophat_amd/csrc/thj_splice_core.h:
// splc::spliced_hit_as<true>, the code thj_k_parse's third instantiation runs per record of a junction-db map) compiled for the
// CPU: records in, hits out.  Beside tests/splicesim, which holds splc::spliced_hit to its own answer for the same records.
//     fusplicesim core <map.bam> <max_report_intron> <contig,contig,...>
//     fusplicesim host <map.bam> <max_report_intron> <contig,contig,...>
// The contigs named on the command line are the ones the run knows (the reference table is frozen after them).  `core` builds the
// target table from the map's header (juncdb_target_from_name, host/thj_hostio.h), prints it,
//     T <tid> <ref_id> <ref_id2> <left> <lsp> <second> <type> <strand>
// and then one line per record, in file order:
//     K <id> <report bits> <ref_id> <left> <flags> <mismatches> <edit_dist> <n_cigar> <cigar x5>     the factory keeps the record
//     D <id> <report bits>                                                                           it drops it
// `host` prints the same K / D lines (report bits 0) from the executables' own host factory, parse_spliced_hit; that one ends the run
// through die() at a fused hit's fifth CIGAR operation, so it is given the quiet records only.
// tests/test_fusplice_core_cpu.py compares both with the Python restatement (tophat_amd/samtext.py: parse_spliced_sam_hits).
#include <cstdio>

#include "../../tophat_amd/csrc/host/thj_hostio.h"
#include "../../tophat_amd/csrc/thj_splice_core.h"

using namespace thjh;

int main(int argc, char** argv) {
    if (argc < 5) { fprintf(stderr, "usage: fusplicesim core|host <map.bam> <max_report_intron> <contig,contig,...>\n"); return 2; }
    const std::string mode = argv[1];
    RefTable rt;
    thj_params p;
    thj_params_default(&p);
    p.max_report_intron = atoi(argv[3]);
    for (auto& n : split(argv[4], ',')) if (!n.empty()) rt.get_id(n);
    rt.freeze();
    AlnReader rd;
    if (!rd.open(argv[2])) return 3;
    if (mode == "host") {
        AlnRec r;
        while (rd.next(r)) {
            Hit h;
            if (!parse_spliced_hit(r, rt, p, h)) printf("D %u 0\n", h.insert_id);
            else printf("K %u 0 %u %d %u %u %u %u %u %u %u %u %u\n", h.insert_id, h.h32.ref_id, h.h32.left, (unsigned)h.h32.flags, (unsigned)h.h32.mismatches,
                        (unsigned)h.h32.edit_dist, (unsigned)h.h32.n_cigar, h.h32.cigar[0], h.h32.cigar[1], h.h32.cigar[2], h.h32.cigar[3], h.h32.cigar[4]);
            fflush(stdout);
        }
        return 0;
    }
    if (mode != "core") return 2;
    std::vector<thj_juncdb_target> tg;
    for (auto& t : rd.targets()) tg.push_back(juncdb_target_from_name(t, rt, false));
    for (size_t t = 0; t < tg.size(); ++t)
        printf("T %zu %u %u %d %d %d %u %u\n", t, tg[t].ref_id, tg[t].ref_id2, tg[t].left, tg[t].lsp, tg[t].second, (unsigned)tg[t].type, (unsigned)tg[t].strand);
    int32_t bs = 0;
    while (const uint8_t* d = rd.next_raw(bs)) {
        // the record on its own, so that a sanitizer sees a read past its end
        std::vector<uint8_t> rec(d, d + bs);
        uint32_t id = 0, rep = 0;
        splc::Hit h;
        if (!splc::spliced_hit_as<true>(rec.data(), (uint32_t)bs, tg.data(), (int64_t)tg.size(), p.max_report_intron, id, h, rep)) printf("D %u %u\n", id, rep);
        else printf("K %u %u %u %d %u %u %u %u %u %u %u %u %u\n", id, rep, h.ref_id, h.left, h.meta & 0xFFu, (h.meta >> 8) & 0xFFu, (h.meta >> 16) & 0xFFu, h.meta >> 24,
                    h.cigar[0], h.cigar[1], h.cigar[2], h.cigar[3], h.cigar[4]);
    }
    return 0;
}
