// TEST-ONLY: the device BAM writer's fusion records (tophat_amd/csrc/thj_bamenc_fusion.h, the code thj_k_bam_shapes<true> and
// thj_k_bam_write_fusion run) compiled for the CPU under tests/hostsim/simt.h -- a wave of 64 fibers per fusion alignment, into an
// output buffer full of stale bytes -- beside the executables' host encoder (encode_aln, host/thj_bamrec.h) on the same batch.
//     xfsim <batch.bin> <out-prefix>
// batch.bin (little-endian): uint32 n_ref, n_aln, n_rows, infl_bytes, names_bytes; the n_ref contig names, NUL-terminated, back to back;
// n_aln thj_aln records; uint32 loc[n_rows]; the reads' BAM records (block_size fields included), record r at loc[r].
// The output header lists the contigs in reverse order, so a contig's target index is not its id - 1.
// Writes <out-prefix>.dev and <out-prefix>.host (the two byte streams) and prints
//     D <size> <read id>        one line per record of the device code
//     H <size> <read id>        one line per record of the host encoder
//     SAME | DIFFERENT
// Exit codes: 0 both agree and the bytes behind the stream are untouched; 1 they differ; 3 a record needs the host encoder (nothing is
// encoded); 2 usage or I/O.  tests/test_bamenc_fusion_cpu.py plants the batch and parses what comes out.
#include <cstdio>

#include "../hostsim/simt.h"
#include "../../tophat_amd/csrc/host/thj_hostio.h"
#include "../../tophat_amd/csrc/host/thj_bamrec.h"
#include "../../tophat_amd/csrc/thj_bamenc_fusion.h"

using namespace thjh;

namespace {
struct SimX { simt::Block* b; int tid, lane, wave; };

bool read_all(const char* fn, std::vector<uint8_t>& out) {
    FILE* f = fopen(fn, "rb");
    if (!f) return false;
    uint8_t buf[65536]; size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
    fclose(f);
    return true;
}
bool write_all(const std::string& fn, const uint8_t* d, size_t n) {
    FILE* f = fopen(fn.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(d, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: xfsim <batch.bin> <out-prefix>\n"); return 2; }
    std::vector<uint8_t> in;
    if (!read_all(argv[1], in) || in.size() < 20) return 2;
    uint32_t h[5];
    memcpy(h, in.data(), 20);
    const uint32_t n_ref = h[0], n_aln = h[1], n_rows = h[2], infl_bytes = h[3], names_bytes = h[4];
    if (in.size() != 20 + (size_t)names_bytes + (size_t)n_aln * sizeof(thj_aln) + (size_t)n_rows * 4 + infl_bytes) { fprintf(stderr, "xfsim: the batch file's size does not match its header\n"); return 2; }
    // every array on its own, so that a sanitizer sees a read or a write past its end
    RefTable rt;
    rt.header_text = "@HD\tVN:1.0\tSO:unsorted\n";
    {
        const char* p = (const char*)in.data() + 20;
        for (uint32_t r = 0; r < n_ref; ++r) { const std::string name(p); rt.get_id(name); p += name.size() + 1; }
        for (uint32_t r = n_ref; r-- > 0;) { rt.sq.emplace_back(rt.names[r], 100000000u); rt.header_text += "@SQ\tSN:" + rt.names[r] + "\tLN:100000000\n"; }
        rt.freeze();
    }
    std::vector<thj_aln> alns(n_aln);
    const uint8_t* at = in.data() + 20 + names_bytes;
    if (n_aln) memcpy(alns.data(), at, (size_t)n_aln * sizeof(thj_aln));
    at += (size_t)n_aln * sizeof(thj_aln);
    std::vector<uint32_t> loc(n_rows);
    if (n_rows) memcpy(loc.data(), at, (size_t)n_rows * 4);
    at += (size_t)n_rows * 4;
    const std::vector<uint8_t> infl(at, at + infl_bytes);
    const std::string prefix = argv[2];
    BamWriter bw;
    if (!bw.open(prefix + ".scratch.bam", rt, "")) return 2;
    std::vector<int32_t> tid_of_ref;
    for (const std::string& name : rt.names) tid_of_ref.push_back(bw.tid_of(name));
    // the contig names as the device holds them
    std::vector<uint8_t> names; std::vector<uint32_t> name_off{0};
    for (const std::string& name : rt.names) { names.insert(names.end(), name.begin(), name.end()); name_off.push_back((uint32_t)names.size()); }

    // ---- the device code: shapes, offsets, records
    std::vector<uint32_t> size1(n_aln), size2(n_aln);
    std::vector<int64_t> rid(n_aln);
    size_t total = 0;
    for (uint32_t i = 0; i < n_aln; ++i) {
        const thj_aln& a = alns[i];
        if (a.read_idx >= n_rows || a.ref_id < 1 || a.ref_id > n_ref || (size_t)loc[a.read_idx] + 36 > infl.size()) { fprintf(stderr, "xfsim: alignment %u points outside the batch\n", i); return 2; }
        const bamenc::FusionShape f = bamenc::fusion_shape(a, infl.data() + loc[a.read_idx] + 4, name_off.data(), (int32_t)n_ref);
        if (f.host_only) { printf("HOST %u\n", i); return 3; }
        size1[i] = f.size1; size2[i] = f.size2; rid[i] = f.rid;
        total += f.size1 + f.size2;
    }
    std::vector<uint8_t> out(total + 64, 0xCD);            // stale bytes under the records, canaries behind them
    size_t off = 0;
    for (uint32_t i = 0; i < n_aln; ++i) {
        const thj_aln& a = alns[i];
        const uint8_t* raw = infl.data() + loc[a.read_idx] + 4;
        if (size2[i] == 0) bamenc::record_write(a, raw, bamenc::record_shape(a, raw), tid_of_ref[a.ref_id - 1], out.data() + off);
        else simt::run_block(64, [&](simt::Block& b, int tid) {
            SimX x{&b, tid, tid & 63, tid >> 6};
            bamenc::fusion_write(x, a, raw, names.data(), name_off.data(), tid_of_ref.data(), out.data() + off);
        });
        off += size1[i] + size2[i];
    }
    bool canary = true;
    for (size_t k = total; k < out.size(); ++k) canary = canary && out[k] == 0xCD;
    for (uint32_t i = 0; i < n_aln; ++i) {
        printf("D %u %lld\n", size1[i], (long long)rid[i]);
        if (size2[i]) printf("D %u %lld\n", size2[i], (long long)rid[i]);
    }

    // ---- the host encoder
    std::vector<uint8_t> d; std::vector<uint32_t> hs; std::vector<long> hr;
    for (uint32_t i = 0; i < n_aln; ++i) {
        Read rd;
        rd.id = alns[i].read_idx; rd.raw = infl.data() + loc[alns[i].read_idx] + 4;
        encode_aln(bw, rt, alns[i], rd, d, hs, hr);
    }
    for (size_t k = 0; k < hs.size(); ++k) printf("H %u %ld\n", hs[k], hr[k]);
    if (!write_all(prefix + ".dev", out.data(), total) || !write_all(prefix + ".host", d.data(), d.size())) return 2;
    const bool same = canary && d.size() == total && (total == 0 || memcmp(d.data(), out.data(), total) == 0);
    if (!canary) fprintf(stderr, "xfsim: the bytes behind the stream were written\n");
    printf("%s\n", same ? "SAME" : "DIFFERENT");
    return same ? 0 : 1;
}
