"""GPU: only each read's best alignments count (thj_juncbed_best_alignments, thj_junctions --best-alignments) against the restatement
(best_ref.py): the hand-worked cases and the crowd of best_cases.py with and without the annotation and the read filter, reads of the
sizes at which a lane-per-record kernel can go wrong, reads across workgroup, grid-stride and add-call boundaries, the BAM route, the
contract, and the executable on both of its routes."""
import os
import subprocess

import numpy as np
import pytest

import best_cases as bc
import best_ref as br
import indelbed_cases as ic
import indelbed_ref as ir
import jbknown_ref as jr
from ingest_cases import cw, record, tag, write_bam
from test_gpu_binaries_reported import BAM_OP, EXE, NIB, members_of, write_ref
from tophat_amd import host

pytestmark = pytest.mark.gpu
NAMES = ["chrA", "chrB"]
TARGETS = tuple((n, len(s)) for n, s in zip(NAMES, bc.GENOME))


def alns(c, lo=0, hi=None, renumber=True):
    """records lo .. hi of the case as an ALN_DTYPE array; read_idx numbers the reads of the call from 0"""
    hi = len(c["recs"]) if hi is None else hi
    a = host.aln_array_from_tuples(c["recs"][lo:hi])
    a["mismatches"] = c["mism"][lo:hi]
    a["AS"] = c["AS"][lo:hi]
    a["flags"] |= np.array([1 if x else 0 for x in c["anti"][lo:hi]], dtype=np.uint8)
    rd = np.array(c["reads"][lo:hi], dtype=np.int64)
    a["read_idx"] = rd - (rd[0] if renumber and len(rd) else 0)
    return a


def run(ctx, c, seqs=None, cuts=(), **over):
    """one consensus through the Context -> (junction rows, insertion rows, deletion rows); cuts: the records go in as several add calls"""
    c = dict(c, **over)
    ctx.juncbed_reset()
    if seqs is not None:
        ctx.juncbed_collect_indels(True)
    if c["known"]:
        ctx.juncbed_known_junctions(c["known"])
    if c["limits"] is not None:
        ctx.juncbed_read_filter(True, *c["limits"])
    if c["best"] is not None:
        ctx.juncbed_best_alignments(True, *c["best"])
    edges = [0] + list(cuts) + [len(c["recs"])]
    for lo, hi in zip(edges, edges[1:]):
        if seqs is not None:
            ctx.juncbed_add_records_seq(alns(c, lo, hi), [ir.ins_letters(r[:5], s) for r, s in zip(c["recs"][lo:hi], seqs[lo:hi])])
        else:
            ctx.juncbed_add_records(alns(c, lo, hi))
    js = ir.junc_rows(ctx.juncbed_finish(c["anchor"]))
    if seqs is None:
        return js, [], []
    ins, dels = ctx.juncbed_indels()
    return js, ir.ins_rows(ins), ir.del_rows(dels)


def want(c, seqs=None, **over):
    c = dict(c, **over)
    return br.consensus(c["recs"], seqs, c["anchor"], c["known"], c["limits"], c["mism"], c["best"], c["reads"], c["AS"], c["anti"])


@pytest.fixture(scope="module")
def ctx():
    with host.Context(0) as c:
        c.upload_genome(host.pack_genome(bc.GENOME))
        yield c


@pytest.fixture(scope="module")
def crowd():
    c = bc.crowd()
    return c, ic.make_seqs(c["recs"], 3)


def test_cases_by_hand(ctx):
    for c in bc.cases():
        seqs = ic.make_seqs(c["recs"], 1)
        got = run(ctx, c, seqs)
        assert (got[0], got[2], len(got[1])) == (c["want_j"], c["want_d"], c["want_i"]), c["label"]
        assert got == want(c, seqs), c["label"]
        assert run(ctx, c)[0] == c["want_j"], c["label"]          # and without the indel sets
    c = [x for x in bc.cases() if x["label"] == "cap_2_of_5"][0]
    run(ctx, c)
    assert ctx.juncbed_best_counts() == (4, 1, 1, 0)


def test_crowd(ctx, crowd):
    c, seqs = crowd
    distinct = sorted({j[:4] for r in c["recs"] for j in ir.rec_juncs(r)})
    seen = set()
    for over in ({}, {"known": distinct[::3]}, {"limits": (0, 2, 2)}, {"known": distinct[1::4], "limits": (0, 2, 2), "anchor": 12, "best": (1, False, 5)}, {"best": (2, True, 6)}):
        got = run(ctx, c, seqs, **over)
        assert got == want(c, seqs, **over), over
        ch = br.choose(c["recs"], c["reads"], c["AS"], c["mism"], c["anti"], over.get("best", c["best"]), over.get("anchor", 8), over.get("known", ()), over.get("limits"))
        assert ctx.juncbed_best_counts() == ch["stats"], over
        seen.add(repr(got))
    assert len(seen) == 5
    # a read lies across a 256-thread workgroup boundary of the per-record kernels
    assert any(s < 256 * k < e for s, e in br.groups(c["reads"]) for k in range(1, 8))
    # the switch off: today's rows
    assert run(ctx, c, seqs, best=None) == jr.consensus(c["recs"], seqs, 8, (), None, c["mism"]) == ir.consensus(c["recs"], seqs)


def big_read(n, seed):
    """a read of n records: deletions at shuffled places, a sixth of them twice (equal under cmp_read_equal), AS 0 or -1"""
    rng = np.random.default_rng(seed)
    base = int(rng.integers(500, 4000))
    places = [int(p) for p in rng.permutation(n)]
    out = []
    for k, p in enumerate(places):
        p = places[k - 1] if k % 6 == 5 else p
        out.append((bc.with_del(base + 30 * p), 0 if rng.integers(0, 4) else -1))
    return out


@pytest.mark.parametrize("cap", (3, 200))
def test_group_sizes(ctx, cap):
    """every read takes the same path (a lane per record that counts over its read): reads of 1, 2, 63, 64, 65 and 130 records, which
    fill a wave exactly, spill one record into the next and span three; the add call's first and last reads are the large ones"""
    sizes = [130, 1, 2, 63, 64, 65, 1, 130]
    c = bc.case("sizes", [big_read(n, 40 + k) for k, n in enumerate(sizes)], best=(cap, False, 6))
    seqs = ic.make_seqs(c["recs"], 2)
    got = run(ctx, c, seqs)
    assert got == want(c, seqs) and len(got[2]) > (100 if cap == 200 else 10)
    ch = br.choose(c["recs"], c["reads"], c["AS"], c["mism"], c["anti"], c["best"])
    assert ctx.juncbed_best_counts() == ch["stats"] and ch["stats"][3] > 20 and (ch["stats"][2] == (5 if cap == 3 else 0))
    # two add calls cut between reads: read numbering and draw order go on
    cut = br.groups(c["reads"])[4][0]
    assert run(ctx, c, seqs, cuts=(cut,)) == got
    if cap == 3:
        assert run(ctx, c, seqs, best=(3, True, 6)) == want(c, seqs, best=(3, True, 6)) != got


def test_a_read_across_the_grid_stride(ctx):
    """the per-record kernels run 4096 workgroups of 256 threads: record 1048576 is the first of the second stride.  A read of 130 tied
    records lies across it, behind 1048500 reads of one unspliced record each (they report, so the generator has drawn 1048500 times)"""
    n_fill, n_big, cap = 1048500, 130, 3
    a = np.zeros(n_fill + n_big + 40, dtype=host.ALN_DTYPE)
    a["ref_id"], a["left"], a["n_cigar"] = 1, 100, 1
    a["cigar"][:, 0] = (bc.M << 28) | 40
    a["read_idx"] = np.arange(len(a))
    big = [bc.with_del(2000 + 30 * k) for k in range(n_big)]
    a[n_fill:n_fill + n_big] = host.aln_array_from_tuples(big)
    a["read_idx"][n_fill:n_fill + n_big] = n_fill
    assert n_fill < 4096 * 256 < n_fill + n_big
    g = br.Mt19937(1)
    for _ in range(n_fill):
        g()
    tie = list(range(n_big))
    while len(tie) > cap:
        del tie[g() % len(tie)]
    ctx.juncbed_reset()
    ctx.juncbed_collect_indels(True)
    ctx.juncbed_best_alignments(True, cap, False, 6)
    ctx.juncbed_add_records(a)
    assert len(ctx.juncbed_finish(8)) == 0
    _ins, dels = ctx.juncbed_indels()
    assert ir.del_rows(dels) == [bc.del_row(2000 + 30 * k) for k in tie]
    assert ctx.juncbed_best_counts() == (n_fill + 1 + 40, 0, 1, 0)


def bam_of(c, seqs):
    out = []
    for k, (r, sq) in enumerate(zip(c["recs"], seqs)):
        nm = c["mism"][k] + sum(ln for op, ln in r[3] if op in (bc.I, bc.D))
        aux = tag("NM", "i", nm) + tag("AS", "i" if k % 2 else "c", c["AS"][k]) + tag("XS", "A", "-" if r[2] else "+")
        out.append(record("q%d" % c["reads"][k], tid=r[0] - 1, pos=r[1], flag=0x10 if c["anti"][k] else 0, cigar=[cw(BAM_OP[op], ln) for op, ln in r[3]],
                          seq=[NIB[x] for x in sq], aux=aux))
    return out


def test_add_bam(ctx, crowd, tmp_path):
    """the crowd as a BAM of 7-record members in pieces of 2: reads sit on piece ends and are kept in one call"""
    c, seqs = crowd
    recs = bam_of(c, seqs)
    bam = write_bam(str(tmp_path / "crowd.bam"), members_of(recs, 7), targets=TARGETS).path
    ctx.bam_contig_names_upload(NAMES)
    by_array = run(ctx, c, seqs)
    for per in (2, 5):
        ctx.juncbed_reset()
        ctx.juncbed_collect_indels(True)
        ctx.juncbed_best_alignments(True, *c["best"])
        assert ctx.juncbed_add_bam(bam, [1, 2], 500000, piece_members=per) == len(recs)
        js = ir.junc_rows(ctx.juncbed_finish(8))
        ins, dels = ctx.juncbed_indels()
        assert (js, ir.ins_rows(ins), ir.del_rows(dels)) == by_array, per
    # a record without AS:i: THJ_EINVAL, nothing counted
    k = 40
    bad = list(recs)
    r = c["recs"][k]
    bad[k] = record("q%d" % c["reads"][k], tid=r[0] - 1, pos=r[1], cigar=[cw(BAM_OP[op], ln) for op, ln in r[3]], seq=[NIB[x] for x in seqs[k]], aux=tag("NM", "i", 0))
    bam2 = write_bam(str(tmp_path / "noas.bam"), members_of(bad, 500), targets=TARGETS).path
    ctx.juncbed_reset()
    ctx.juncbed_best_alignments(True, *c["best"])
    with pytest.raises(host.ThjError, match=r"\(-1\).*AS:i"):
        ctx.juncbed_add_bam(bam2, [1, 2], 500000)
    assert len(ctx.juncbed_finish(8)) == 0 and ctx.juncbed_best_counts()[0] == 0
    # without the switch the same file is taken as ever
    ctx.juncbed_reset()
    assert ctx.juncbed_add_bam(bam2, [1, 2], 500000) > 0


def test_contract(ctx):
    c = [x for x in bc.cases() if x["label"] == "support4"][0]
    plain = jr.consensus(c["recs"], None, 8)[0]
    assert plain != c["want_j"]
    # after the first add: THJ_ESTATE
    ctx.juncbed_reset()
    ctx.juncbed_add_records(alns(c))
    with pytest.raises(host.ThjError, match=r"\(-5\).*records were added already"):
        ctx.juncbed_best_alignments(True)
    assert ir.junc_rows(ctx.juncbed_finish(8)) == plain
    # on, then a reset: off again
    assert run(ctx, c)[0] == c["want_j"]
    assert run(ctx, c, best=None)[0] == plain and ctx.juncbed_best_counts() == (0, 0, 0, 0)
    # taken back before the first add
    ctx.juncbed_reset()
    ctx.juncbed_best_alignments(True)
    ctx.juncbed_best_alignments(False)
    ctx.juncbed_add_records(alns(c))
    assert ir.junc_rows(ctx.juncbed_finish(8)) == plain
    # what is not built says so
    ctx.juncbed_reset()
    ctx.juncbed_best_alignments(True)
    with pytest.raises(host.ThjError, match=r"\(-1\).*not built"):
        ctx.juncbed_collect_fusions(True)
    with pytest.raises(host.ThjError, match=r"\(-1\).*not built"):
        ctx.juncbed_add_span()
    ctx.juncbed_reset()
    ctx.juncbed_collect_fusions(True)
    with pytest.raises(host.ThjError, match=r"\(-1\).*not built"):
        ctx.juncbed_best_alignments(True)
    # read_idx must not fall, and stays below the call's size; nothing is counted
    for bad in ("falls", "large"):
        ctx.juncbed_reset()
        ctx.juncbed_best_alignments(True)
        a = alns(c)
        if bad == "falls":
            a["read_idx"][2] = 0
        else:
            a["read_idx"][-1] = len(a)
        with pytest.raises(host.ThjError, match=r"\(-1\).*read_idx"):
            ctx.juncbed_add_records(a)
        assert len(ctx.juncbed_finish(8)) == 0
    with pytest.raises(host.ThjError, match=r"\(-1\)"):
        ctx.juncbed_reset()
        ctx.juncbed_best_alignments(True, 0, False, 6)


# ---------------------------------------------------------------- the executable

def thj_junctions(tmp_path, tag_, ref_fa, hdr, bam, extra, env, ok=True):
    d = tmp_path / tag_
    d.mkdir()
    args = [EXE, "--sam-header", str(hdr), "--insertions-out", str(d / "insertions.bed"), "--deletions-out", str(d / "deletions.bed")] + extra
    r = subprocess.run(args + [str(ref_fa), str(d / "junctions.bed"), str(bam)], capture_output=True, text=True, env=dict(os.environ, **env), timeout=120)
    if not ok:
        return r
    assert r.returncode == 0, (tag_, r.stderr[-1000:])
    return {f: open(d / f).read() for f in ("junctions.bed", "insertions.bed", "deletions.bed")}, r.stderr


def text(js, ins, dels):
    return {"junctions.bed": ir.junctions_bed(js, NAMES), "insertions.bed": ir.insertions_bed(ins, NAMES), "deletions.bed": ir.deletions_bed(dels, NAMES)}


ROUTES = (("host", {"THJ_HOST_INGEST": "1"}), ("dev", {"THJ_DEVICE_INGEST": "1", "THJ_PIECE_MEMBERS": "3"}))


def test_thj_junctions_best_alignments(tmp_path, crowd):
    c, seqs = crowd
    ref_fa, hdr = write_ref(tmp_path, NAMES, bc.GENOME)
    bam = write_bam(str(tmp_path / "crowd.bam"), members_of(bam_of(c, seqs), 9), targets=TARGETS).path
    settings = {
        "plain": ([], None),
        "options_without_the_switch": (["--max-multihits", "1", "--suppress-hits", "--bowtie2-max-penalty", "3"], None),
        "best": (["--best-alignments"], (20, False, 6)),
        "cap2": (["--best-alignments", "--max-multihits", "2"], (2, False, 6)),
        "suppressed": (["--best-alignments", "--max-multihits", "2", "--suppress-hits", "--bowtie2-max-penalty", "5"], (2, True, 5)),
    }
    wants = {}
    for name, (extra, best) in settings.items():
        wants[name] = text(*want(c, seqs, best=best))
        for route, env in ROUTES:
            got, err = thj_junctions(tmp_path, name + "_" + route, ref_fa, hdr, bam, extra, env)
            assert ("parsed on the device" if route == "dev" else "read on the host (THJ_HOST_INGEST)") in err
            assert got == wants[name], (name, route)
            if best:
                st = br.choose(c["recs"], c["reads"], c["AS"], c["mism"], c["anti"], best)["stats"]
                assert "best alignments: %d reads, %d lost alignments to the choice, %d over --max-multihits %d" % (st[0], st[1], st[2], best[0]) in err
                assert "%d alignments counted once as first-pass duplicates" % st[3] in err
    # without the switch: the files of the existing restatements, byte for byte
    assert wants["plain"] == wants["options_without_the_switch"] == text(*ir.consensus(c["recs"], seqs))
    assert len({repr(wants[k]) for k in ("plain", "best", "cap2", "suppressed")}) == 4


def test_thj_junctions_refusals(tmp_path, crowd):
    c, seqs = crowd
    ref_fa, hdr = write_ref(tmp_path, NAMES, bc.GENOME)
    recs = bam_of(c, seqs)[:60]
    bam = write_bam(str(tmp_path / "some.bam"), members_of(recs, 9), targets=TARGETS).path
    r = thj_junctions(tmp_path, "fus", ref_fa, hdr, bam, ["--best-alignments", "--fusions-out", str(tmp_path / "fusions.out")], {}, ok=False)
    assert r.returncode != 0 and "--best-alignments beside --fusions-out is not built" in r.stderr
    r = thj_junctions(tmp_path, "sec", ref_fa, hdr, bam, ["--best-alignments", "--report-secondary-alignments"], {}, ok=False)
    assert r.returncode != 0 and "--best-alignments beside --report-secondary-alignments is not built" in r.stderr
    k = 7
    rc = c["recs"][k]
    recs[k] = record("noscore", tid=rc[0] - 1, pos=rc[1], cigar=[cw(BAM_OP[op], ln) for op, ln in rc[3]], seq=[NIB[x] for x in seqs[k]], aux=tag("NM", "i", 0))
    bam = write_bam(str(tmp_path / "noas.bam"), members_of(recs, 9), targets=TARGETS).path
    for route, env in ROUTES:
        r = thj_junctions(tmp_path, "noas_" + route, ref_fa, hdr, bam, ["--best-alignments"], env, ok=False)
        assert r.returncode != 0 and "AS:i" in r.stderr, route
    assert "noscore" in thj_junctions(tmp_path, "noas_named", ref_fa, hdr, bam, ["--best-alignments"], ROUTES[0][1], ok=False).stderr
