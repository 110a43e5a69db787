"""CPU: fusions.out of tophat_reports' consensus pass.  The Python restatement of the reference (tests/fusionsout_ref.py) against
lines written out by hand for a small two-contig genome, difference() on pairs worked by hand, the walker header the device
kernels run (jbw::fusion, jbw::unsplit_span of tophat_amd/csrc/thj_jb_walk.h) compiled for the CPU (tests/fusionsim), and the
rules of the two passes one by one."""
import os
import subprocess

import numpy as np

import fusionsout_cases as fc
import fusionsout_ref as fr
from locked_make import locked_make
from tophat_amd import host

HERE = os.path.dirname(os.path.abspath(__file__))
M, m, N, FF, FR, RF, RR = fc.M, fc.m, fc.N, fc.FF, fc.FR, fc.RF, fc.RR
_RC = str.maketrans("ACGTN", "TGCAN")

# fc.directions(): FF, FR (beside a run of N), RF, RR, the FF whose key swaps (chrB 349 -> chrA 2500 becomes chrA 2500 - chrB 349),
# the one 34 bases from chrA's start (no strings, no values), the intra-contig one that swaps.  Counts, unsupport, extents and symm
# are worked out in the comments of test_hand_written_lines.
EXPECTED = [
    'chrA-chrB\t1059\t500\tff\t2\t0\t0\t3\t60\t55\t0.000000\t@\t14 26 39 53 66 \t@\tATCCCGCCGTTTTACCGCGAACTGTCGAATGCCACATCAACGTCAATAGT CCCTGCTGTGGAGTGAGTCCGCTCGGCGTTTCGATCCCCCGGGACTTCGG\t@\tGGCAGTCGTCCCGTGTCCCCTGCAGACCGATAACGATCTGAGTGCCCTGT TGCGATAGCAAGTGCACAATCTTGGACGCATGTTTGCACAACCGGCTCTT\t@\t2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 1 1 1 1 1 1 1 1 1 1 \t@\t2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 2 1 1 1 1 1 1 1 1 1 1 \t@\t\n',
    'chrA-chrB\t1199\t800\tfr\t1\t0\t0\t1\t50\t50\t0.000000\t@\t15 32 43 57 68 \t@\tTAGTCGCCTTCCTCAGCACGCACGGGAGTGNNNNGCCCCGAATCATTAAA TTCTGGAGAAAGGTGGTGAGTTATGTGAGCGCAGGGAAGATCTTGCTAGC\t@\tTTGGAAGACTAATTTAGTAGTATTTCTGATGGTCAAGTCCGTGGTCTAAG TGGTNNCATGCCCTCCCCGGTGACTTCTACTAATACCTAGGGCTAAGTGG\t@\t1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 \t@\t1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 \t@\t\n',
    'chrA-chrB\t656\t900\trf\t1\t0\t0\t1\t45\t55\t5.000000\t@\t14 26 42 52 63 \t@\tGACGCAGATTTCGTAAAATGATCCCAGGTTTACATGCCCAGCAAAAAGTC ATCGATCCTTGCGGCCTTCAGAGGCCTTGCAGTACCCGCCGAGTATCGCT\t@\tAAAAGATAGTGAGGTATGGTTGAGTGTTCGCACCTTTAAGACGCCACAAG GGGCACCGCACCTCCCTCTGAGTGGAGCCGTTAGAGAGCATGTGTGTCCC\t@\t1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 0 0 0 0 0 \t@\t1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 \t@\t\n',
    'chrA-chrB\t1951\t1500\trr\t1\t0\t0\t1\t50\t50\t0.000000\t@\t11 25 34 49 63 \t@\tGTCATACACTCTGCGTATGCATGCCCGAAATCGGCGACTCATATATGTCC GCCCCGTCTTCGTTCGTCCAGAGATGGCGTCGCGGATGAGTGATGGTGTA\t@\tACCACTGTAGAACGCGGGCTTTCTCCGACAAGTGTTTTATCACTTACGTC CCCAGAGCATGCTCCACTGCTGCGTACTGAAGCACGAACAGCGGTTAGTT\t@\t1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 \t@\t1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 \t@\t\n',
    'chrA-chrB\t2500\t349\tff\t1\t0\t0\t0\t50\t50\t0.000000\t@\t12 22 35 47 60 \t@\tTCGTTCAATGTAGCTACACTATAACACTGCAGATCGGACAGTTTGATCGC AGACACTGTCTGCCCTGCCCCGTTCGAGAGATCGGCACTGGCTAGAGCGC\t@\tTCCTATGCTAAGTCAAACAGTAAGTGTATAGCACCGGTAATTCCTGATAT CTAAATATTCCCTAAACTGGACCATCACCACGAGTAGATAAGGATGCCGG\t@\t1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 \t@\t1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 \t@\t\n',
    'chrA-chrB\t34\t1000\tff\t1\t0\t0\t0\t25\t75\t25.000000\t@\t\t@\t \t@\t \t@\t1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 \t@\t1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 \t@\t\n',
    'chrA-chrA\t150\t2329\tff\t1\t0\t0\t2\t30\t70\t20.000000\t@\t13 28 40 54 68 \t@\tCATGGTACCATGAGGACACCTATAAATAATGAGTATTTGGTTGTGGATCG GGAAAGGGGACGTGGTGCAATATAGCCCGCAGTCCTCGGCACATTGCCTG\t@\tAAAAGGCTCCCTTCCAATAGTAGGATACTCCGCTCACTCTTCCTGCTATC CTAGCGTGGTATATCTTCACCCGAGGTTACGGCTGTGGAAGGCTTCCATT\t@\t1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 \t@\t1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 \t@\t\n',
]


def test_hand_written_lines():
    recs = fc.renumber(fc.directions())
    rows = fr.fusions(recs, fc.GENOME)
    text = fr.fusions_out(rows, fc.NAMES)
    for line in EXPECTED:
        assert line in text, line[:40]
    assert text.count("\n") == 11
    a, b = fc.GENOME
    by = {r[0]: r for r in rows}
    # FF 1059 / 500: two reads (anchors 60|40 and 40|55): left_bases 2 up to k = 39, 1 up to 49; right_bases the same: symm 0.
    # unsupport 3: 100M at chrA 1000 ([1020, 1080] holds 1059), 100M at chrB 450 ([470, 530] holds 500: the mirror), 2250M at chrA 100
    r = by[(1, 2, 1059, 500, 7)]
    assert r[1:5] == (2, 3, 60, 55) and r[5] == (2,) * 40 + (1,) * 10 and r[6] == (2,) * 40 + (1,) * 10
    assert r[7] == a[1010:1110] and r[8] == b[450:550]                                   # :245, :253
    r = by[(1, 2, 1199, 800, 8)]
    assert r[7] == a[1150:1250] and "NNNN" in r[7] and r[8] == b[751:851].translate(_RC)[::-1] and "NN" in r[8]        # :245, :249-250
    r = by[(1, 2, 656, 900, 9)]
    assert r[7] == a[606:706].translate(_RC)[::-1] and r[8] == b[850:950]                # :241-242, :253
    assert r[5] == (1,) * 45 + (0,) * 5 and r[6] == (1,) * 50                            # symm = 5 * (0 - 1)^2 = 5
    r = by[(1, 2, 1951, 1500, 10)]
    assert r[7] == a[1901:2001].translate(_RC)[::-1] and r[8] == b[1451:1551].translate(_RC)[::-1]
    assert by[(1, 2, 2500, 349, 7)][7] == a[2451:2551] and by[(1, 2, 2500, 349, 7)][2] == 0
    assert by[(1, 2, 34, 1000, 7)][7:] == ("", "", ())
    assert by[(1, 2, 1549, 1960, 7)][7:] == ("", "", ()) and len(by[(1, 2, 1549, 1950, 7)][7]) == 100
    # intra-contig, both ends inside the 2250M read: 2 from it (429 also from the 100M at 380: 3)
    assert by[(1, 1, 150, 2329, 7)][2] == 2 and by[(1, 1, 429, 2200, 7)][2] == 3
    for r in rows:                                            # the five values: the centred 20 .. 100 bases
        if r[7]:
            assert r[9] == tuple(fr.difference(r[7][p:100 - p], r[8][p:100 - p]) for p in (40, 30, 20, 10, 0))


def test_difference_by_hand():
    assert fr.difference("ACGTACGTAC", "ACGTACGTAC") == 0
    assert fr.difference("ACGTACGTAC", "ACGTTCGTAC") == 1                                # one substitution on the diagonal
    # a one-base shift: the diagonal pays for every column, the path one row off pays 2 for its first step and then nothing, and it
    # may end anywhere in the last row or column
    assert fr.difference("AACCGGTTAC", "ACCGGTTACG") == 2
    assert fr.difference("ACGT", "ACGTA") == 0 and fr.difference("", "") == 10000        # unequal lengths: 0; nothing to compare: the start value
    # two rows by hand: first = "AC", second = "CA": (i, j) = (0,0) 1, (1,0) 2, (0,1) 2, (1,1) min(2 + 2, 2 + 2, 1 + 1) = 2; ends: 2, 2, 2
    assert fr.difference("AC", "CA") == 2


def test_walker_header_equals_the_restatement():
    locked_make(os.path.join(HERE, "fusionsim"))
    recs = fc.walker_cases() + fc.directions() + fc.crowd()
    got = subprocess.run([os.path.join(HERE, "fusionsim", "fusionsim")], input=fc.sim_input(recs), capture_output=True, text=True, check=True).stdout
    want = fc.sim_expected(recs, fr)
    assert got == want
    assert want.count("\nF ") > 300 and "F 1 2 4294967290 500 7 10 40 1" in want        # 5 - 10 - 1 wraps below 0
    assert "F 1 2 4294967295 500 7 0 40 0" in want and "F 1 2 141 500 9 40 0 0" in want  # first op, last op
    assert "F 1 1 7 4294967291 10 10 30 1" in want                                       # 0xFFFFFFF0 + 10 + 1 is not below 7: the key swaps
    assert "F 1 1 700 700 7 50 50 1" in want                                             # its own mirror


def _rows(recs, **kw):
    return {r[0]: r for r in fr.fusions(fc.renumber(recs), fc.GENOME, **kw)}


def _fus(read, a=60, b=40, ed=0, left_break=1059):
    return (1, left_break + 1 - a, False, [(M, a), (FF, 500), (M, b)], 2, read, ed)


def test_properties_of_the_two_passes():
    K = (1, 2, 1059, 500, 7)
    # anchors: 19 fails, 20 passes, on either side
    assert K not in _rows([_fus(0, 19, 40)]) and K not in _rows([_fus(0, 40, 19)]) and K in _rows([_fus(0, 20, 20)])
    assert K in _rows([_fus(0, 19, 40)], anchor=19)
    # left_pos 49, 50 and 51 against the 50 bins
    for lp, want in ((49, (1,) * 49 + (0,)), (50, (1,) * 50), (51, (1,) * 50)):
        assert _rows([_fus(0, lp, 40)])[K][5] == want and _rows([_fus(0, lp, 40)])[K][3] == lp
    # three records of one read with multireads 2: none counts; two do
    assert _rows([_fus(0), _fus(0), _fus(0)]) == {} and _rows([_fus(0), _fus(0)])[K][1] == 2
    assert _rows([_fus(0), _fus(0), _fus(0)], multi=3)[K][1] == 3
    # a read of three records of which the junction filter drops one (its junction's anchor is 5): pass 1 skips the read, pass 2
    # counts its two others; the fusion is in the pass-1 set through another read
    dropped = (1, 200, False, [(M, 40), (N, 100), (M, 5)], 0, 0, 0)
    rows = _rows([_fus(0, 30, 30), _fus(0, 30, 30), dropped, _fus(1)])
    assert rows[K][1] == 3 and rows[K][3] == 60
    # ... and when no other read puts a fusion into the pass-1 set, the reference's second pass runs like its first: a count, nothing else
    rows = _rows([_fus(0, 30, 30), _fus(0, 30, 30), dropped])
    assert rows[K][1:5] == (2, 0, 0, 0) and rows[K][5] == (0,) * 50 and rows[K][7:] == ("", "", ())
    # edit_dist 2 passes, 3 does not
    assert _rows([_fus(0, ed=2)])[K][1] == 1 and _rows([_fus(0, ed=3)]) == {} and _rows([_fus(0, ed=3)], mism=3)[K][1] == 1

    def un(left, ln=100, read=5, ed=0, cig=None):
        return (1, left, False, cig or [(M, ln)], 0, read, ed)
    # unsupport at E.left == L, == R, and one outside each: L = left + 20, R = left + 100 - 20
    assert [_rows([_fus(0), un(l)])[K][2] for l in (1039, 1040, 979, 978)] == [1, 0, 1, 0]
    # read_len 39 vs 40 (the interval of a 40-base read is the single position left + 20)
    assert _rows([_fus(0), un(1039, 40)])[K][2] == 1 and _rows([_fus(0), un(1039, 39)])[K][2] == 0
    # a spliced record never unsupports; one over the edit distance neither; nor the third alignment of a read
    assert _rows([_fus(0), un(1000, cig=[(M, 70), (N, 100), (M, 30)])])[K][2] == 0
    assert _rows([_fus(0), un(1000, ed=3)])[K][2] == 0
    assert _rows([_fus(0), un(1000), un(1000), un(1000)])[K][2] == 0 and _rows([_fus(0), un(1000), un(1000)])[K][2] == 2
    # an intra-contig fusion with both ends inside one read counts 2
    intra = (1, 371, False, [(M, 30), (FF, 600), (M, 70)], 1, 0, 0)
    assert _rows([intra, un(300, 400)])[(1, 1, 400, 600, 7)][2] == 2
    # a fusion seen only in pass 1 (the filter drops its record) gets unsupport but no row
    only1 = (1, 919, False, [(M, 5), (N, 100), (M, 36), (FF, 500), (M, 40)], 2, 0, 0)
    assert fr.rec_fusion(only1)[0] == K and _rows([only1, un(1000)]) == {}


def test_text_from_the_stat_array_is_the_restatements():
    """host.fusions_out_text over a FUSSTAT_DTYPE array filled from the restatement's rows: the same bytes, symm in float32"""
    rows = fr.fusions(fc.crowd(), fc.GENOME)
    a = np.zeros(len(rows), dtype=host.FUSSTAT_DTYPE)
    for x, (k, count, unsup, le, re, lb, rb, s1, s2, diffs) in zip(a, rows):
        x["ref_id1"], x["ref_id2"], x["left"], x["right"], x["dir"] = k
        x["count"], x["unsupport"], x["left_ext"], x["right_ext"], x["n_diffs"] = count, unsup, le, re, len(diffs)
        x["diffs"][:len(diffs)] = diffs
        x["left_bases"], x["right_bases"], x["seq1"], x["seq2"] = lb, rb, s1.encode(), s2.encode()
    assert fr.stat_rows(a) == rows and len(rows) >= 5
    assert host.fusions_out_text(a, fc.NAMES) == fr.fusions_out(rows, fc.NAMES)
    assert any(float(l.split("\t")[10]) not in (0.0, 5.0, 20.0) for l in fr.fusions_out(rows, fc.NAMES).splitlines())
