// TEST-ONLY: the record core of thj_juncbed_add_bam (tophat_amd/csrc/thj_reported_core.h: rpt::reported_record, the code
// thj_k_parse_reported runs per record of a BAM of reported alignments) compiled for the CPU: records in, one line per record out.
//     reportedsim <in.bam> <max_report_intron> <indels 0|1> <fusions 0|1> <contig,contig,...>
// The contigs named on the command line are the ones the run knows, ref_id 1, 2, ... in that order; the file's targets are resolved
// against them (0 = unknown).  Per record, in file order:
//     K <ref_id> <left> <flags> <edit_dist> <n_cigar> <cigar x16> <inserted letters, - for none> <head>     the core keeps the record
//     D <report bits>                                                                                       it does not
// head = 1 when the record opens a read's run among the kept records (rpt::same_read against the kept record before it).
// tests/test_reported_core_cpu.py compares the lines with the Python restatement of thj_junctions' host reader (tests/reported_ref.py).
#include <algorithm>
#include <cstdio>

#include "../../tophat_amd/csrc/host/thj_hostio.h"
#include "../../tophat_amd/csrc/thj_reported_core.h"

using namespace thjh;

int main(int argc, char** argv) {
    if (argc < 6) { fprintf(stderr, "usage: reportedsim <in.bam> <max_report_intron> <indels 0|1> <fusions 0|1> <contig,contig,...>\n"); return 2; }
    const std::vector<std::string> names = split(argv[5], ',');
    // the name table as thj_bam_contig_names_upload lays it out
    std::vector<uint8_t> blob; std::vector<uint32_t> off{0};
    for (auto& n : names) { blob.insert(blob.end(), n.begin(), n.end()); off.push_back((uint32_t)blob.size()); }
    std::vector<uint32_t> sorted(names.size());
    for (size_t r = 0; r < names.size(); ++r) sorted[r] = (uint32_t)r;
    std::sort(sorted.begin(), sorted.end(), [&](uint32_t x, uint32_t y) { return names[x] != names[y] ? names[x] < names[y] : x < y; });
    blob.push_back(0);
    AlnReader rd;
    if (!rd.open(argv[1]) || !rd.is_bam()) return 3;
    std::vector<uint32_t> tid2ref;
    for (auto& t : rd.targets()) { const auto it = std::find(names.begin(), names.end(), t); tid2ref.push_back(it == names.end() ? 0u : (uint32_t)(it - names.begin()) + 1u); }
    rpt::Cfg cfg;
    cfg.tid2ref = tid2ref.data(); cfg.n_tid = (uint32_t)tid2ref.size(); cfg.max_report_intron = atoi(argv[2]);
    cfg.indels = atoi(argv[3]) != 0; cfg.fusions = atoi(argv[4]) != 0;
    cfg.names = rpt::Names{blob.data(), off.data(), sorted.data(), (int32_t)names.size()};
    std::vector<uint8_t> prev;
    int32_t bs = 0;
    while (const uint8_t* d = rd.next_raw(bs)) {
        // the record on its own, so that a sanitizer sees a read past its end
        std::vector<uint8_t> rec(d, d + bs);
        thj_aln a; memset(&a, 0xEE, sizeof a);
        rpt::Seq s; uint32_t n_ins = 0, rep = 0;
        if (!rpt::reported_record(rec.data(), (uint32_t)bs, cfg, a, s, n_ins, rep)) { printf("D %u\n", rep); continue; }
        printf("K %u %d %u %u %u", a.ref_id, a.left, (unsigned)a.flags, (unsigned)a.edit_dist, (unsigned)a.n_cigar);
        for (int i = 0; i < 16; ++i) printf(" %u", a.cigar[i]);
        std::vector<uint8_t> letters(n_ins + 1, 0);
        if (cfg.indels) rpt::ins_letters(rec.data(), a, s, letters.data());
        printf(" %s %d\n", n_ins ? (const char*)letters.data() : "-", prev.empty() || !rpt::same_read(prev.data(), rec.data()) ? 1 : 0);
        prev = rec;
    }
    return 0;
}
