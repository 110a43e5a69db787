"""GPU: the unmapped-read files and the align-summary counters on the device (thj_juncbed_collect_unmapped, thj_juncbed_read_numbers,
thj_juncbed_report_unmapped_bam, thj_juncbed_align_stats) against the hand-worked cases and the restatement (unmapped_ref.py: the
reference's loop), byte for byte with counters equal: record shapes, every outcome row single-end and paired, the crowds; reads files of
1, 63, 64, 65 and 257 records, a piece boundary between any two records, one read in 64 written and every read written, the counting
call against the writing call, numbers from the QNAMEs of a BAM of alignments, the contract, and that the switch changes nothing else."""
import ctypes as C

import numpy as np
import pytest

import best_cases as bc
import pair_cases as pc
import unmapped_cases as uc
import unmapped_ref as ur
from ingest_cases import write_bam
from test_gpu_accepted import NAMES, TARGETS, anti_of, planted, raw_records
from test_gpu_best import alns
from test_gpu_binaries_reported import members_of
from test_gpu_pair import n_inserts, side_alns
from test_unmapped_cpu import by_number, ref_paired, ref_single
from tophat_amd import host

pytestmark = pytest.mark.gpu
EMPTY = dict(recs=[], reads=[], AS=[], mism=[], anti=[], numbers=[], known=[], limits=None, anchor=8, best=(20, False, 6))


def reads_bam(records, per_member=7):
    return write_bam(None, members_of(records, per_member), targets=()).data


@pytest.fixture(scope="module")
def ctx():
    with host.Context(0) as c:
        c.upload_genome(host.pack_genome(bc.GENOME))
        c.bam_contig_names_upload(NAMES)
        yield c


def arm(ctx, c, best, pair=None, max_report_intron=500000, unmapped=True):
    ctx.juncbed_reset()
    if c["known"]:
        ctx.juncbed_known_junctions(c["known"])
    if c["limits"] is not None:
        ctx.juncbed_read_filter(True, *c["limits"])
    ctx.juncbed_best_alignments(True, *best)
    if pair is not None:
        ctx.juncbed_pair_alignments(True, *pair)
    if unmapped:
        ctx.juncbed_collect_unmapped(True, max_report_intron)


def single(ctx, c, best=None, file=None, per_member=7, per=None, cuts=(), unmapped=True):
    """a single-end consensus from host arrays -> (the unmapped records' stream, their sizes, the counters, the junction rows)"""
    best = best or c["best"]
    arm(ctx, c, best, unmapped=unmapped)
    edges = [0] + list(cuts) + [len(c["recs"])]
    for lo, hi in zip(edges, edges[1:]):
        if hi > lo:
            ctx.juncbed_add_records(alns(c, lo, hi))
            if unmapped:
                ctx.juncbed_read_numbers([c["numbers"][k] for k in sorted(set(c["reads"][lo:hi]))])
    rows = ctx.juncbed_finish(c["anchor"])
    if not unmapped:
        return None, None, None, rows
    stream, sizes = ctx.juncbed_report_unmapped_bam(0, reads_bam(file if file is not None else c["file"], per_member), piece_members=per)
    return stream, sizes, ctx.juncbed_align_stats(), rows


def paired(ctx, c, best=None, pair=None, per_member=7, per=None, cuts=(), unmapped=True):
    best, pair = best or c["best"], pair or c["pair"]
    arm(ctx, c, best, pair, c.get("max_report_intron", 500000), unmapped)
    edges = [0] + list(cuts) + [n_inserts(c)]
    for lo, hi in zip(edges, edges[1:]):
        ctx.juncbed_add_pairs(side_alns(c["L"], lo, hi), side_alns(c["R"], lo, hi))
        if unmapped:
            nums = sorted({k for S in (c["L"], c["R"]) for k in S["reads"] if lo <= k < hi})
            ctx.juncbed_read_numbers([c["numbers"][k] for k in nums])
    rows = ctx.juncbed_finish(c["anchor"])
    if not unmapped:
        return None, None, None, rows, ctx.juncbed_pair_counts()
    left, lsizes = ctx.juncbed_report_unmapped_bam(0, reads_bam(c["left_file"], per_member), piece_members=per)
    right, rsizes = ctx.juncbed_report_unmapped_bam(1, reads_bam(c["right_file"], per_member), piece_members=per)
    return (left, lsizes), (right, rsizes), ctx.juncbed_align_stats(), rows, ctx.juncbed_pair_counts()


def test_record_shapes(ctx):
    cs = uc.shape_cases()
    stream, sizes, stats, _rows = single(ctx, EMPTY, file=[raw for _l, raw, _w in cs])
    want = [w for _l, _r, w in cs]
    assert sizes == [len(w) for w in want]
    at = 0
    for (label, _raw, w) in cs:
        assert stream[at:at + len(w)] == w, label
        at += len(w)
    assert stats == [0, len(cs)] + [0] * 13


def test_single_end_outcomes(ctx):
    c = uc.single_case()
    recs = by_number(c["file"])
    for suppress, (written, want_stats) in c["want"].items():
        want = [ur.write_unmapped_record(ur.QRead(recs[k][4:])) for k in written]
        stream, sizes, stats, _rows = single(ctx, c, (2, suppress, 6))
        assert (stream, sizes, stats) == (b"".join(want), [len(w) for w in want], want_stats), suppress


def test_paired_outcomes(ctx):
    c = uc.paired_case()
    lrec, rrec = by_number(c["left_file"]), by_number(c["right_file"])
    for (mixed, discordant, best), (lw, rw, want_stats) in c["want"].items():
        pair = c["pair"][:3] + (mixed, discordant)
        want_l = b"".join(ur.write_unmapped_record(ur.QRead(lrec[k][4:])) for k in lw)
        want_r = b"".join(ur.write_unmapped_record(ur.QRead(rrec[k][4:])) for k in rw)
        left, right, stats, _rows, _pc = paired(ctx, c, best, pair)
        assert (left[0], right[0], stats) == (want_l, want_r, want_stats), (mixed, discordant, best)


def test_single_crowd(ctx):
    c = uc.single_crowd()
    for best, cuts, per in (((2, False, 6), (), None), ((2, True, 6), (c["reads"].index(100), c["reads"].index(101)), 2)):
        left, _r, want_stats = ref_single(c, best)
        stream, sizes, stats, _rows = single(ctx, c, best, cuts=cuts, per=per)
        assert sizes == [len(w) for w in left] and stream == b"".join(left) and stats == want_stats, best


def test_paired_crowd(ctx):
    c = uc.paired_crowd()
    for pair, best, cuts in (((200, 20, 10000000, False, False), (2, False, 6), ()), ((200, 20, 10000000, True, False), (2, False, 6), (97, 98, 200)),
                             ((200, 20, 900, False, True), (2, True, 6), ()), ((150, 30, 10000000, True, True), (1, True, 5), ())):
        wl, wr, want_stats = ref_paired(c, best, pair)
        left, right, stats, _rows, _pc = paired(ctx, c, best, pair, cuts=cuts)
        assert left[0] == b"".join(wl) and right[0] == b"".join(wr) and stats == want_stats, (pair, best)
        assert left[1] == [len(w) for w in wl] and right[1] == [len(w) for w in wr]
    c = uc.paired_crowd(mate_bits=False)
    wl, wr, want_stats = ref_paired(c, (2, False, 6), (200, 20, 10000000, True, False))
    left, right, stats, _rows, _pc = paired(ctx, c, (2, False, 6), (200, 20, 10000000, True, False))
    assert (left[0], right[0], stats) == (b"".join(wl), b"".join(wr), want_stats)


def group_case(n, no_group_every):
    """n reads in a file, each with one alignment except every no_group_every-th (0: none has one)"""
    has = [k for k in range(n) if no_group_every and k % no_group_every != no_group_every - 1]
    c = bc.case("sizes", [[(bc.plain(100 + 7 * k, 40), 0)] for k in has])
    c["numbers"] = [k + 1 for k in has]
    rng = np.random.default_rng(n)
    c["file"] = [uc.read_shape(rng, k + 1, 4, True) for k in range(n)]
    return c


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_reads_file_sizes(ctx, n):
    """a file of n records: every read written (none has a group), and one read in 64 without a group"""
    for every in (0, 64):
        c = group_case(n, every)
        left, _r, want_stats = ref_single(c)
        stream, sizes, stats, _rows = single(ctx, c, per_member=50)
        assert (stream, sizes, stats) == (b"".join(left), [len(w) for w in left], want_stats), (n, every)
        assert every or len(sizes) == sum(1 for r in c["file"] if b"ZTAM" not in r)


def test_piece_boundaries_and_the_counting_call(ctx):
    """one record a member: pieces of 1, 2, 3 and 5 members put a boundary between any two records; the counting call gives the writing call's
    figures and keeps nothing"""
    c = uc.single_case()
    c["file"] = c["file"] + [uc.rd(k, zn="t%d" % k, flag=4 | (0x10 if k % 2 else 0), seq=[k % 16] * (k % 7)) for k in range(21, 30)]
    left, _r, want_stats = ref_single(c)
    for per in (1, 2, 3, 5, None):
        stream, sizes, stats, _rows = single(ctx, c, per_member=1, per=per)
        assert (stream, sizes, stats) == (b"".join(left), [len(w) for w in left], want_stats), per
    arm(ctx, c, c["best"])
    ctx.juncbed_add_records(alns(c))
    ctx.juncbed_read_numbers(c["numbers"])
    ctx.juncbed_finish(8)
    bam = reads_bam(c["file"], 1)
    assert ctx.juncbed_report_unmapped_bam(0, bam, piece_members=3, count_only=True) == (len(left), len(b"".join(left)))
    assert ctx.juncbed_report_unmapped_bam(0, bam, piece_members=3, count_only=True) == (len(left), len(b"".join(left)))      # (nothing was kept of the first)
    stream, sizes = ctx.juncbed_report_unmapped_bam(0, bam, piece_members=3)
    assert stream == b"".join(left) and ctx.juncbed_align_stats() == want_stats


def test_resume_point(ctx):
    """more_follows: the resume point is the piece's end, whatever follows"""
    c = uc.single_case()
    arm(ctx, c, c["best"])
    ctx.juncbed_add_records(alns(c))
    ctx.juncbed_read_numbers(c["numbers"])
    ctx.juncbed_finish(8)
    w = write_bam(None, members_of(c["file"], 3), targets=())
    offs, m, skip, _t = host.bam_layout(w.data)
    buf = np.frombuffer(w.data + bytes(64), dtype=np.uint8)
    n, rm, rs, tot = C.c_int64(), C.c_uint32(), C.c_uint32(), C.c_int64()
    sizes = np.zeros(16, dtype=np.uint32)
    piece = host.CBamPiece(buf.ctypes.data + offs[m], offs[m + 2] - offs[m], skip, 0, None)
    rc = ctx.lib.thj_juncbed_report_unmapped_bam(ctx._ctx, 0, C.byref(piece), 1, C.byref(n), C.byref(rm), C.byref(rs), sizes.ctypes.data_as(C.c_void_p), C.c_int64(16), C.byref(tot))
    assert rc == 0 and (rm.value, rs.value) == (2, 0) and n.value == 2          # reads 5 (written), 7 (ZT M), 10, 11, 12 (aligned), 13 (written)
    with pytest.raises(host.ThjError, match="has not been reported to its end"):
        ctx.juncbed_align_stats()
    piece = host.CBamPiece(buf.ctypes.data + offs[m + 2], offs[-1] - offs[m + 2], 0, 0, None)
    rc = ctx.lib.thj_juncbed_report_unmapped_bam(ctx._ctx, 0, C.byref(piece), 0, C.byref(n), C.byref(rm), C.byref(rs), sizes.ctypes.data_as(C.c_void_p), C.c_int64(16), C.byref(tot))
    assert rc == 0 and n.value == 2
    assert ctx.juncbed_align_stats() == c["want"][False][1]


def test_numbers_from_a_bam_and_nothing_else_changes(ctx):
    """thj_juncbed_add_bam takes the numbers from the QNAMEs; with the switch on the bed rows and accepted_hits come out as without it"""
    c = planted([1, 2, 16, 17, 21, 1, 3])
    numbers = [10 + 3 * k for k in range(7)]
    raws = raw_records(c, names=["%d" % numbers[r] for r in c["reads"]])
    bam = write_bam(None, members_of(raws, 7), targets=TARGETS).data
    file = [uc.rd(k, zn="n%d" % k, zt="M" if k % 5 == 0 else None) for k in range(8, 32)]
    out = {}
    for on in (False, True):
        ctx.juncbed_reset()
        ctx.juncbed_best_alignments(True, *c["best"])
        ctx.juncbed_collect_accepted(True, 1, "", [0, 1])
        if on:
            ctx.juncbed_collect_unmapped(True, 500000)
        ctx.juncbed_add_bam(bam, [1, 2], 500000, piece_members=5)
        rows = ctx.juncbed_finish(8)
        sizes, total = ctx.juncbed_report_bam(bam, [1, 2], 500000, piece_members=5)
        out[on] = (rows.tobytes(), sizes, ctx.bam_stream_download(total), ctx.juncbed_best_counts())
    assert out[False] == out[True]
    stream, sizes = ctx.juncbed_report_unmapped_bam(0, reads_bam(file))
    cc = dict(c, anti=anti_of(raws), numbers=numbers, known=[], limits=None, anchor=8)
    left, _r, want_stats = ur.walk(cc, None, [r[4:] for r in file], None, numbers, c["best"])
    assert stream == b"".join(left) and ctx.juncbed_align_stats() == want_stats
    # ... and a paired consensus: bed rows and pair counts
    p = uc.paired_case()
    off, on = paired(ctx, p, unmapped=False), paired(ctx, p)
    assert (off[3].tobytes(), off[4]) == (on[3].tobytes(), on[4])
    # QNAMEs that are no numbers
    bad = write_bam(None, members_of(raw_records(c), 7), targets=TARGETS).data
    ctx.juncbed_reset()
    ctx.juncbed_best_alignments(True, *c["best"])
    ctx.juncbed_collect_unmapped(True, 500000)
    with pytest.raises(host.ThjError, match="not digits"):
        ctx.juncbed_add_bam(bad, [1, 2], 500000)


def test_beside_the_other_switches(ctx):
    """the indel sets and the reported pairs armed beside it: the unmapped files and the counters are what they are alone"""
    c = uc.paired_case()
    (mixed, discordant, best), (lw, rw, want_stats) = next(iter(c["want"].items()))
    pair = c["pair"][:3] + (mixed, discordant)
    arm(ctx, c, best, pair, c["max_report_intron"])
    ctx.juncbed_collect_indels(True)
    ctx.juncbed_collect_accepted(True, 1, "", [0, 1], pairs=True)
    ctx.juncbed_add_pairs(side_alns(c["L"], 0, n_inserts(c)), side_alns(c["R"], 0, n_inserts(c)))
    ctx.juncbed_read_numbers(c["numbers"])
    ctx.juncbed_finish(c["anchor"])
    lrec, rrec = by_number(c["left_file"]), by_number(c["right_file"])
    left, _s = ctx.juncbed_report_unmapped_bam(0, reads_bam(c["left_file"]))
    right, _s = ctx.juncbed_report_unmapped_bam(1, reads_bam(c["right_file"]))
    assert left == b"".join(ur.write_unmapped_record(ur.QRead(lrec[k][4:])) for k in lw)
    assert right == b"".join(ur.write_unmapped_record(ur.QRead(rrec[k][4:])) for k in rw)
    assert ctx.juncbed_align_stats() == want_stats


def test_loud_reads_files(ctx):
    for label, file, text in uc.loud_cases():
        with pytest.raises(host.ThjError, match=text):
            single(ctx, EMPTY, file=file)
    # numbers that fall across two pieces
    with pytest.raises(host.ThjError, match="fall or repeat"):
        single(ctx, EMPTY, file=[uc.rd(7), uc.rd(8), uc.rd(8)], per_member=2, per=1)
    # a read without mate bits on an insert one of whose sides has only records over the limits left
    c = pc.pcase("ambiguous", [([(pc.L0, 0)], [(uc.Rr(200), 0, 5)])], limits=(2, 2, 2))
    c.update(numbers=[4], left_file=[uc.rd(4, flag=4)], right_file=[uc.rd(4, flag=0x85)], max_report_intron=500)
    with pytest.raises(host.ThjError, match="not built"):
        paired(ctx, c)
    c["left_file"] = [uc.rd(4, flag=0x45)]
    wl, wr, want_stats = ref_paired(c)
    left, right, stats, _rows, _pc = paired(ctx, c)
    assert (left[0], right[0], stats) == (b"".join(wl), b"".join(wr), want_stats)


def test_contract(ctx):
    c = uc.single_case()
    bam = reads_bam(c["file"])
    ctx.juncbed_reset()
    with pytest.raises(host.ThjError, match=r"\(-5\).*best alignments are not being chosen"):
        ctx.juncbed_collect_unmapped(True, 500000)
    with pytest.raises(host.ThjError, match=r"\(-5\).*not armed"):
        ctx.juncbed_report_unmapped_bam(0, bam)
    with pytest.raises(host.ThjError, match=r"\(-5\).*not armed"):
        ctx.juncbed_align_stats()
    with pytest.raises(host.ThjError, match=r"\(-5\).*not being collected"):
        ctx.juncbed_read_numbers([1])
    arm(ctx, c, c["best"])
    with pytest.raises(host.ThjError, match=r"\(-5\).*thj_juncbed_finish first"):
        ctx.juncbed_report_unmapped_bam(0, bam)
    ctx.juncbed_add_records(alns(c))
    with pytest.raises(host.ThjError, match=r"\(-5\).*records were added already"):
        ctx.juncbed_collect_unmapped(True, 500000)
    with pytest.raises(host.ThjError, match=r"\(-5\).*still waits for its read numbers"):
        ctx.juncbed_add_records(alns(c))
    for bad, text in (([10, 11, 12], "3 numbers, the add call before has 4 reads"), ([10, 11, 11, 13], "fall or repeat"), ([10, 9, 12, 13], "fall or repeat"), ([0, 1, 2, 3], "read number 0")):
        with pytest.raises(host.ThjError, match=r"\(-1\).*" + text):
            ctx.juncbed_read_numbers(bad)
    ctx.juncbed_finish(8)
    with pytest.raises(host.ThjError, match=r"\(-5\).*have no read numbers"):
        ctx.juncbed_report_unmapped_bam(0, bam)
    ctx.juncbed_read_numbers(c["numbers"])
    with pytest.raises(host.ThjError, match=r"\(-5\).*no add call waits"):
        ctx.juncbed_read_numbers([50])
    ctx.juncbed_finish(8)
    with pytest.raises(host.ThjError, match=r"\(-1\).*side 1"):
        ctx.juncbed_report_unmapped_bam(1, bam)
    with pytest.raises(host.ThjError, match=r"\(-5\).*has not been reported to its end"):
        ctx.juncbed_align_stats()
    ctx.juncbed_report_unmapped_bam(0, bam)
    with pytest.raises(host.ThjError, match=r"\(-5\).*reported already"):
        ctx.juncbed_report_unmapped_bam(0, bam)
    assert ctx.juncbed_align_stats() == c["want"][False][1]
    # a finish again opens the replay again; a read with a group that no reads file holds is loud
    ctx.juncbed_finish(8)
    ctx.juncbed_report_unmapped_bam(0, reads_bam([r for r in c["file"] if by_number([r]).get(11) is None]))
    with pytest.raises(host.ThjError, match=r"\(-1\).*1 left reads with alignments were met in no reads file"):
        ctx.juncbed_align_stats()
    # numbers rise across add calls; thj_juncbed_best_alignments again, and a reset, turn the switch off
    arm(ctx, c, c["best"])
    ctx.juncbed_add_records(alns(c, 0, 3))
    ctx.juncbed_read_numbers([10, 11])
    ctx.juncbed_add_records(alns(c, 3, 7))
    with pytest.raises(host.ThjError, match=r"\(-1\).*fall or repeat"):
        ctx.juncbed_read_numbers([11, 13])
    ctx.juncbed_reset()
    ctx.juncbed_best_alignments(True, *c["best"])
    ctx.juncbed_collect_unmapped(True, 500000)
    ctx.juncbed_best_alignments(True, *c["best"])
    ctx.juncbed_add_records(alns(c))
    ctx.juncbed_add_records(alns(c))                           # (no numbers are waited for)
    ctx.juncbed_finish(8)
    with pytest.raises(host.ThjError, match=r"\(-5\).*not armed"):
        ctx.juncbed_report_unmapped_bam(0, bam)
    # device arrays beside the switch: not built
    arm(ctx, c, c["best"])
    with pytest.raises(host.ThjError, match=r"\(-1\).*not built"):
        rc = ctx.lib.thj_juncbed_add_records(ctx._ctx, C.c_void_p(8), C.c_int64(1), C.c_int32(1))
        if rc:
            raise host.ThjError("thj_juncbed_add_records failed (%d): %s" % (rc, ctx.lib.thj_last_error().decode()))
