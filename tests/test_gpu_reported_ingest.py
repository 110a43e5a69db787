"""GPU: thj_juncbed_add_bam (host.Context.juncbed_add_bam) -- a BAM of reported alignments inflated, parsed, ordered and numbered by
read on the device -- against the same consensus fed with HOST records: what the Python restatement of thj_junctions' host reader
(reported_ref.py) makes of the same bytes, through juncbed_add_records / juncbed_add_records_seq.  Junction, insertion, deletion and
fusion rows must be equal row for row, in every combination of "indels collected" and "fusions collected"."""
import numpy as np
import pytest

import reported_cases as rc
import reported_ref as rr
from ingest_cases import D, I, M, MAX_INTRON, N, cw, record, tag, write_bam
from tophat_amd import host

pytestmark = pytest.mark.gpu
EINVAL, ESTATE, EFALLBACK = -1, -5, -6


def _genome():
    rng = np.random.default_rng(5)
    return ["".join(rng.choice(list("ACGT"), size=12000)) for _ in rc.KNOWN]


@pytest.fixture(scope="module")
def ctx():
    with host.Context(0) as c:
        c.upload_genome(host.pack_genome(_genome()))
        c.bam_contig_names_upload(rc.KNOWN)
        yield c


def _begin(ctx, mode):
    ind, fus = rc.MODES[mode]
    ctx.juncbed_reset()
    if ind:
        ctx.juncbed_collect_indels(True)
    if fus:
        ctx.juncbed_collect_fusions(True, 5, 255, 8)
    return ind, fus


def _rows(ctx):
    js = ctx.juncbed_finish(1)
    ins, dels = ctx.juncbed_indels()
    return js.tobytes(), ins.tobytes(), dels.tobytes(), ctx.juncbed_fusions().tobytes(), (len(js), len(ins), len(dels))


def _add_restated(ctx, mode, files):
    """the restatement's records of every file (one add call per file, as the host route does) -> records added"""
    ind, fus = rc.MODES[mode]
    total = 0
    for w in files:
        kept, idx = rr.parse_all(w.records_from(0), rc.TID2REF, rc.name_id, MAX_INTRON, ind, fus)
        a = np.zeros(len(kept), dtype=host.ALN_DTYPE)
        for i, k in enumerate(kept):
            a[i]["ref_id"], a[i]["left"], a[i]["flags"], a[i]["edit_dist"], a[i]["n_cigar"], a[i]["read_idx"] = k.ref_id, k.left, k.flags, k.edit_dist, k.n_cigar, idx[i]
            a[i]["cigar"][:] = k.cigar
        if len(a) and ind:
            ctx.juncbed_add_records_seq(a, [k.letters for k in kept])
        elif len(a):
            ctx.juncbed_add_records(a)
        total += len(a)
    return total


def _want(ctx, mode, files):
    _begin(ctx, mode)
    n = _add_restated(ctx, mode, files)
    return n, _rows(ctx)


def _got(ctx, mode, files, piece_members=None):
    _begin(ctx, mode)
    n = sum(ctx.juncbed_add_bam(w.data, rc.TID2REF, MAX_INTRON, piece_members) for w in files)
    return n, _rows(ctx)


def _same(ctx, mode, files, piece_members=None):
    want = _want(ctx, mode, files)
    got = _got(ctx, mode, files, piece_members)
    assert got[0] == want[0], "records counted"
    assert got[1][4] == want[1][4], "row counts (junctions, insertions, deletions)"
    assert got[1] == want[1]
    return want


@pytest.mark.parametrize("mode", range(4))
def test_planted_records(ctx, mode):
    """every quiet case of reported_cases, in one member, over 2 and 5 members, with the header in a member of its own, and cut into
    pieces of 1 and 3 members"""
    cases = rc.quiet(mode)
    n_kept = sum(1 for c in cases if c[1][mode] == "K")
    for per_member, header_alone, pieces in ((None, False, None), ((len(cases) + 1) // 2, False, 1), ((len(cases) + 4) // 5, True, 3), ((len(cases) + 4) // 5, False, 1)):
        w = rc.write(None, cases, per_member, header_alone=header_alone)
        n, rows = _same(ctx, mode, [w], pieces)
        assert n == n_kept
        assert rows[4][0] >= 1 and (not rc.MODES[mode][0] or (rows[4][1] >= 1 and rows[4][2] >= 1)) and (not rc.MODES[mode][1] or len(rows[3]) > 0)


def _many(n):
    """n small records of one member: spliced, with an insertion, with a deletion, a fusion pair, plain ones of reads with 1-3 alignments"""
    out = []
    for k in range(n):
        kind, pos, name = k % 5, 500 + 37 * (k % 11), "r%d" % (k // 3)
        if kind == 0:
            out.append(record(name, pos=pos, cigar=[cw(M, 10), cw(N, 200 + k % 7), cw(M, 15)], seq=rc.seq(25), aux=tag("XS", "A", "-+"[k & 1]) + tag("NM", "C", k % 4)))
        elif kind == 1:
            out.append(record(name, tid=1, pos=pos, cigar=[cw(M, 9 + k % 3), cw(I, 1 + k % 3), cw(M, 10)], seq=rc.seq(24, 10, (1, 2, 4, 8, 15)[k % 5])))
        elif kind == 2:
            out.append(record(name, pos=pos, cigar=[cw(M, 12), cw(D, 1 + k % 4), cw(M, 13)], seq=rc.seq(25)))
        elif kind == 3:
            out.append(record(name, pos=pos, cigar=[cw(M, 25)], seq=rc.seq(25), aux=rc.fus("20M%dF12%s" % (3000 + k % 9, "Mm"[k & 1]), pos=pos + 1) + tag("NM", "C", k % 3)))
        else:
            out.append(record(name, pos=pos, flag=0x40 if k % 2 else 0x80, cigar=[cw(M, 50)], seq=rc.seq(50)))
    return out


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_records_of_one_member(ctx, n):
    w = write_bam(None, [(_many(n), 6)], targets=rc.TARGETS)
    for mode in (0, 3):
        cnt, rows = _same(ctx, mode, [w])
        assert cnt == (n if mode == 3 else sum(1 for k in range(n) if k % 5 == 0))


def test_empty_members_in_the_middle_and_at_the_end(ctx):
    recs = _many(40)
    w = write_bam(None, [(recs[:13], 6), ([], 6), (recs[13:30], 6), ([], 6), ([], 6), (recs[30:], 6), ([], 6)], targets=rc.TARGETS)
    assert w.member_len.count(0) == 4
    for pieces in (None, 1, 2, 3):
        assert _same(ctx, 3, [w], pieces)[0] == 40


def _reads(runs, pos0=2000):
    """fusion alignments (the first of their two records): runs[k] alignments of read k, one after the other, each with a fusion of its own"""
    return [record("q%d" % k, pos=pos0, cigar=[cw(M, 32)], seq=rc.seq(32), aux=rc.fus("20M%dF12M" % (3000 + 40 * k + 7 * j), pos=pos0 + 100 * k + 10 * j + 1) + tag("NM", "C", j))
            for k, n in enumerate(runs) for j in range(n)]


def _fusion_run(ctx, multi, add):
    ctx.juncbed_reset()
    ctx.juncbed_collect_fusions(True, 5, 255, multi)
    n = add()
    return n, _rows(ctx)


def test_a_reads_alignments_across_a_member_edge_and_a_piece_cut(ctx):
    """--fusion-multireads counts a read's records: with multireads 2 the reads with three alignments are skipped, wherever the members
    and the pieces are cut"""
    recs = _reads([1, 2, 3, 1, 3, 2])                      # 12 records
    # a piece covers piece_members members of new ground, so a run of three records over three members needs pieces of three
    for cut, sizes in (([4], (1, 2)), ([5], (1, 2)), ([4, 5], (2, 3)), ([3, 6, 8], (1, 2)), ([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], (3, 4))):
        edges = [0] + cut + [len(recs)]
        w = write_bam(None, [(recs[a:b], 6) for a, b in zip(edges, edges[1:])], targets=rc.TARGETS)
        want = _fusion_run(ctx, 2, lambda: _add_restated(ctx, 2, [w]))
        all_reads = _fusion_run(ctx, 8, lambda: _add_restated(ctx, 2, [w]))
        assert want[0] == 12 and want[1][3] != all_reads[1][3], "the reads with three alignments make a difference"
        for pieces in (None,) + sizes:
            assert _fusion_run(ctx, 2, lambda: ctx.juncbed_add_bam(w.data, rc.TID2REF, MAX_INTRON, pieces)) == want, (cut, pieces)


def test_a_piece_whose_only_run_is_its_last(ctx):
    recs = _reads([3, 1])
    w = write_bam(None, [(recs[:2], 6), (recs[2:], 6)], targets=rc.TARGETS)
    _begin(ctx, 2)
    with pytest.raises(host.ThjError, match="more alignments than a piece holds") as e:
        ctx.juncbed_add_bam(w.data, rc.TID2REF, MAX_INTRON, 1)
    assert e.value.code == EFALLBACK
    _begin(ctx, 0)                                           # without fusion collection nothing has to stay together (and nothing here is kept)
    assert ctx.juncbed_add_bam(w.data, rc.TID2REF, MAX_INTRON, 1) == 0
    _same(ctx, 2, [w], 2)


@pytest.mark.parametrize("first", ["AC", "GT"])
def test_first_insertion_in_file_order_keeps_its_letters(ctx, first):
    second = "GT" if first == "AC" else "AC"

    def ins(name, letters):
        s = rc.seq(25)
        s[10:12] = [rc.codes(ch)[0] for ch in letters]
        return record(name, pos=3000, cigar=[cw(M, 10), cw(I, 2), cw(M, 13)], seq=s)
    pad = _many(20)
    w = write_bam(None, [(pad[:10] + [ins("a", first)], 6), (pad[10:] + [ins("b", second)], 6)], targets=rc.TARGETS)
    for pieces in (None, 1):
        _same(ctx, 1, [w], pieces)
        ins_rows, _dels = ctx.juncbed_indels()
        mine = [r for r in ins_rows if int(r["ref_id"]) == 1 and 3000 <= int(r["left"]) <= 3020 and int(r["len"]) == 2]
        assert len(mine) == 1 and int(mine[0]["support"]) == 2 and mine[0]["bases"][:2].decode() == first


@pytest.mark.parametrize("label", sorted(rc.LOUD_WHAT))
def test_loud_records_count_nothing(ctx, label):
    """THJ_EINVAL with a message that says which, and the consensus as it was: the next finish equals a run without that call"""
    message = {"malformed": "malformed BAM record", "xf_ops": "more than 15 CIGAR operations", "cigar_ops": "more than 16 CIGAR operations",
               "ins_range": "insertion lies outside", "ins_long": "insertion of more than 16 bases", "ins_letter": "other than A, C, G, T and N"}[rc.LOUD_WHAT[label]]
    case = [c for c in rc.CASES if c[0] == label][0]
    mode = case[1].index("L") if case[1] != "LLLL" else 3
    good = rc.write(None, rc.quiet(mode)[:30])
    bad = write_bam(None, [(_many(10), 6), (_many(7) + [case[2]] + _many(5), 6)], targets=rc.TARGETS)
    want = _want(ctx, mode, [good])
    _begin(ctx, mode)
    ctx.juncbed_add_bam(good.data, rc.TID2REF, MAX_INTRON)
    with pytest.raises(host.ThjError, match=message) as e:
        ctx.juncbed_add_bam(bad.data, rc.TID2REF, MAX_INTRON)
    assert e.value.code == EINVAL
    assert _rows(ctx) == want[1]


def test_a_straddling_record_wants_the_host(ctx):
    recs = _many(12)
    w = write_bam(None, [(recs[:6] + [recs[6][:20]], 6), ([recs[6][20:]] + recs[7:], 6)], targets=rc.TARGETS)
    _begin(ctx, 0)
    with pytest.raises(host.ThjError, match="straddle") as e:
        ctx.juncbed_add_bam(w.data, rc.TID2REF, MAX_INTRON)
    assert e.value.code == EFALLBACK


def test_names_must_be_there():
    with host.Context(0) as c:
        c.upload_genome(host.pack_genome(_genome()))
        c.juncbed_reset()
        with pytest.raises(host.ThjError, match="thj_bam_contig_names_upload") as e:
            c.juncbed_add_bam(write_bam(None, [(_many(5), 6)], targets=rc.TARGETS).data, rc.TID2REF, MAX_INTRON)
        assert e.value.code == ESTATE
