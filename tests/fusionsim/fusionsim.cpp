// TEST-ONLY: the fusion walkers of the consensus pass (jbw::fusion and jbw::unsplit_span of tophat_amd/csrc/thj_jb_walk.h, the code
// the device kernels run) compiled for the CPU.  Reads records from stdin, one a line:
//     <ref_id> <left> <ref_id2> <n> <op> <len> ... (n pairs)
// and prints for every record:
//     R <record>
//     F <ref1> <ref2> <left> <right> <dir> <left_pos> <right_pos> <inner>       (a record with a fusion op)
//     U <read_len> <right> <qualifies>
// tests/test_fusionsout_cpu.py compares that with the Python restatement of the reference (tests/fusionsout_ref.py).
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
        jbw::FusionSite s;
        if (jbw::fusion(cigar, n, (int32_t)left, (uint32_t)ref, s))
            printf("F %u %u %u %u %u %u %u %d\n", s.ref1, s.ref2, s.left, s.right, s.dir, s.left_pos, s.right_pos, s.inner ? 1 : 0);
        const jbw::UnsplitSpan u = jbw::unsplit_span(cigar, n, (int32_t)left);
        printf("U %u %u %d\n", u.read_len, u.right, u.qualifies ? 1 : 0);
    }
    return 0;
}
