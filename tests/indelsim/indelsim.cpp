// TEST-ONLY: the record walkers of the junction / indel consensus (tophat_amd/csrc/thj_jb_walk.h, the code the device kernels run)
// compiled for the CPU.  Reads records from stdin, one a line:
//     <ref_id> <left> <ref_id2> <n> <op> <len> ... (n pairs)
// and prints every occurrence of every record, record by record:
//     J <ref> <left> <right> <left_extent> <right_extent>
//     D <ref> <left> <right> <left_extent> <right_extent> <op index>
//     I <ref> <left> <length> <position in the read> <left_extent> <right_extent> <op index>
// tests/test_indelbed_cpu.py compares that with the Python restatement of the reference (tests/indelbed_ref.py).
#include <cstdio>
#include <cstring>

#include "../../tophat_amd/csrc/thj_jb_walk.h"

int main() {
    long long ref, left, ref2; int n;
    int rec = 0;
    while (scanf("%lld %lld %lld %d", &ref, &left, &ref2, &n) == 4) {
        uint32_t cigar[16];
        memset(cigar, 0, sizeof cigar);
        if (n < 0 || n > 16) { fprintf(stderr, "record %d: %d ops\n", rec, n); return 1; }
        for (int c = 0; c < n; ++c) {
            unsigned op, len;
            if (scanf("%u %u", &op, &len) != 2) { fprintf(stderr, "record %d: short line\n", rec); return 1; }
            cigar[c] = (op << 28) | (len & 0x0FFFFFFFu);
        }
        if (ref2) cigar[15] = (uint32_t)ref2;
        printf("R %d\n", rec++);
        jbw::juncs(cigar, n, (int32_t)left, (uint32_t)ref, [](uint32_t r, uint32_t l, uint32_t rt, uint32_t le, uint32_t re) { printf("J %u %u %u %u %u\n", r, l, rt, le, re); });
        jbw::dels(cigar, n, (int32_t)left, (uint32_t)ref, [](uint32_t r, uint32_t l, uint32_t rt, uint32_t le, uint32_t re, int c) { printf("D %u %u %u %u %u %d\n", r, l, rt, le, re, c); });
        jbw::inss(cigar, n, (int32_t)left, (uint32_t)ref, [](uint32_t r, uint32_t l, uint32_t len, uint32_t rp, uint32_t le, uint32_t re, int c) { printf("I %u %u %u %u %u %u %d\n", r, l, len, rp, le, re, c); });
    }
    return 0;
}
