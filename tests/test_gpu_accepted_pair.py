"""GPU: accepted_hits.bam for graded inserts through the ABI (thj_juncbed_collect_accepted_pairs beside thj_juncbed_pair_alignments,
thj_juncbed_report_pairs_bam) against the restatement (accepted_pair_ref.py on pair_ref.py's choice), byte for byte: the hand-worked cases,
the crowd, pair lists and single sides on both sides of the counting / std::sort seam, inserts across workgroup edges, several add calls,
records at every byte alignment, a long run of unchanged tags, the count-only mode, the contract, and a single-end consensus afterwards."""
import struct

import pytest

import accepted_pair_cases as apc
import accepted_pair_ref as apr
import best_cases as bc
import best_ref as br
import pair_cases as pc
from best_cases import plain
from ingest_cases import tag, write_bam
from test_gpu_accepted import cfg_of as single_cfg, expected as single_expected, planted, raw_records, through_ctx as single_through_ctx, TARGETS
from test_gpu_binaries_reported import members_of
from test_gpu_pair import n_inserts, side_alns
from tophat_amd import host

pytestmark = pytest.mark.gpu
L0 = apc.L0


@pytest.fixture(scope="module")
def ctx():
    with host.Context(0) as c:
        c.upload_genome(host.pack_genome(pc.GENOME))
        c.bam_contig_names_upload(apc.NAMES)
        yield c


def raws_in(c, raw, s, lo, hi):
    return [raw[s][k] for k, num in enumerate(c[s]["reads"]) if lo <= num < hi]


def arm(ctx, c, cfg):
    ctx.juncbed_reset()
    if c.get("known"):
        ctx.juncbed_known_junctions(c["known"])
    if c.get("limits") is not None:
        ctx.juncbed_read_filter(True, *c["limits"])
    ctx.juncbed_best_alignments(True, *c["best"])
    ctx.juncbed_pair_alignments(True, *c["pair"])
    ctx.juncbed_collect_accepted(True, cfg["library_type"], cfg["rg"], [cfg["header"].index(n) if n in cfg["header"] else -1 for n in cfg["names"]], pairs=True)


def through_ctx(ctx, c, raw, cfg, cuts=(), count_first=False):
    """the whole call sequence -> (the stream, the record sizes)"""
    arm(ctx, c, cfg)
    edges = [0] + list(cuts) + [n_inserts(c)]
    for lo, hi in zip(edges, edges[1:]):
        ctx.juncbed_add_pairs(side_alns(c["L"], lo, hi), side_alns(c["R"], lo, hi))
    ctx.juncbed_finish(c.get("anchor", 8))
    stream, sizes = b"", []
    for lo, hi in zip(edges, edges[1:]):
        lr, rr = raws_in(c, raw, "L", lo, hi), raws_in(c, raw, "R", lo, hi)
        if count_first:
            counted = ctx.juncbed_report_pairs_bam(lr, rr, count_only=True)
        before = len(stream)
        stream, s = ctx.juncbed_report_pairs_bam(lr, rr)
        if count_first:
            assert counted == (len(s), sum(s)) and len(stream) - before == sum(s)
        sizes += s
    return stream, sizes


def check(ctx, c, raw, cfg, want=None, **kw):
    if want is None:
        want, _seen = apr.accepted(c, raw, cfg)
    stream, sizes = through_ctx(ctx, c, raw, cfg, **kw)
    assert sizes == [len(w) for w in want]
    assert stream == b"".join(want)
    return want


def test_cases_by_hand(ctx):
    for c in apc.cases():
        raw = apc.raw_of(c)
        assert check(ctx, c, raw, c["cfg"], want=c["want"], count_first=True) == apr.accepted(c, raw, c["cfg"])[0], c["label"]
    for n in range(1, 7):
        c = apc.mapq_case(n)
        want = check(ctx, c, apc.raw_of(c), c["cfg"], want=c["want"])
        assert len(want) == 2 * n and all(w[4 + 9] == apc.MAPQ[n] for w in want)


@pytest.fixture(scope="module")
def crowd():
    c = apc.crowd()
    return c, apc.raw_of(c, apc.crowd_extra)


def test_crowd(ctx, crowd):
    c, raw = crowd
    cfg = apc.cfg_of(2, "grp")
    want, seen = apr.accepted(c, raw, cfg)
    assert seen["pairs"] > 100 and seen["sides"] > 50 and 0 < seen["happy"] < seen["pairs"]
    check(ctx, c, raw, cfg, want=want, count_first=True)
    # two and three add calls: an insert's neighbours lie on both sides of every seam; the visit order and the draws go on
    check(ctx, c, raw, cfg, want=want, cuts=(137,))
    check(ctx, c, raw, cfg, want=want, cuts=(1, 150))
    # discordant pairs instead of mixed alignments, the other library type, no read group
    c2 = dict(c, pair=(200, 20, 10000000, False, True))
    check(ctx, c2, raw, apc.cfg_of(3))


def tied_rights(n):
    """n right records behind L0, all inside the window, all tied"""
    assert n % 7 and n <= 40
    return [(plain(1220 + k * 7 % n, 40), 0) for k in range(n)]


@pytest.mark.parametrize("n", (1, 2, 15, 16, 17, 40))
def test_list_sizes(ctx, n):
    """pair lists of n entries (max_multihits raised): up to 16 the device counts index_vector, beyond the host's std::sort orders it; the same for a
    left read that goes alone with n tied alignments; a small insert before and behind"""
    small = ([(L0, 0)], [(apc.W, 0)])
    alone = ([(plain(900 + 3 * (k * 7 % n), 40), 0) for k in range(n)], [])
    c = apc.pcase("sizes", [small, ([(L0, 0)], tied_rights(n)), alone, small], best=(100, False, 6), pair=apc.MIXED)
    raw = apc.raw_of(c)
    want, seen = apr.accepted(c, raw, apc.cfg_of())
    assert seen["big"] == (2 if n > 16 else 0) and len(want) == 2 + 2 * n + n + 2
    check(ctx, c, raw, apc.cfg_of(), want=want)


@pytest.mark.parametrize("n", (255, 256, 257))
def test_inserts_across_a_workgroup(ctx, n):
    """a lane per insert in workgroups of 256: the last inserts are a 1 x 2 (a record written twice) and a singleton"""
    ins = [([(plain(1000 + k, 40), 0)], [(plain(1240 + k, 40), 0)]) for k in range(n - 2)] + [([(L0, 0)], [(apc.W, 0), (plain(1245, 40), 0)]), ([], [(apc.W, 0)])]
    c = apc.pcase("edge", ins, pair=apc.MIXED)
    raw = apc.raw_of(c)
    want = check(ctx, c, raw, apc.cfg_of())
    assert len(want) == 2 * (n - 2) + 4 + 1


def test_output_records_across_a_workgroup(ctx):
    """the per-record kernels: 128 inserts of 1 x 1 are one workgroup's worth of output records, a singleton is one more"""
    ins = [([(plain(1000 + k, 40), 0)], [(plain(1240 + k, 40), 0)]) for k in range(128)] + [([(L0, 0)], [])]
    c = apc.pcase("edge", ins, pair=apc.MIXED)
    assert len(check(ctx, c, apc.raw_of(c), apc.cfg_of())) == 257


def test_byte_alignments_and_a_long_tag_run(ctx):
    """records of odd l_seq whose names make them start at all four byte alignments, one with more than 256 bytes of unchanged tags"""
    ins = [([(plain(1000 + k, 39), 0)], [(plain(1240 + k, 39), 0)]) for k in range(8)]
    c = apc.pcase("align", ins)
    names = ["q" * (1 + k) for k in range(8)]
    raw = {s: [apc.raw_record(names[k], r, S["anti"][k], 0, tag("ZL", "Z", "x" * 300) + tag("YC", "C", 7) if k == 3 else b"") for k, r in enumerate(S["recs"])]
           for s, S in (("L", c["L"]), ("R", c["R"]))}
    starts = {sum(len(r) for r in raw["L"][:k]) % 4 for k in range(8)} | {sum(len(r) for r in raw["R"][:k]) % 4 for k in range(8)}
    assert starts == {0, 1, 2, 3}
    want = check(ctx, c, raw, apc.cfg_of(2, "g"))
    assert any(len(w) > 400 for w in want) and all(struct.unpack_from("<i", w, 4 + 16)[0] == 39 for w in want)


# ---------------------------------------------------------------- the contract

@pytest.mark.parametrize("lc", apc.loud_cases(), ids=[x[0] for x in apc.loud_cases()])
def test_loud_cases(ctx, lc):
    _label, c, extra, patch, header, word = lc
    raw = apc.raw_of(c, extra)
    if patch:
        patch(raw)
    cfg = apc.cfg_of(header=header)
    with pytest.raises(host.ThjError, match=r"\(-1\)") as e:
        through_ctx(ctx, c, raw, cfg)
    assert word in str(e.value)


def test_call_order(ctx):
    c = apc.pcase("order", [([(L0, 0)], [(apc.W, 0)]), ([(L0, 0)], [(apc.W, 0), (plain(1245, 40), 0)])])
    raw, cfg = apc.raw_of(c), apc.cfg_of()
    L, R = side_alns(c["L"], 0, 2), side_alns(c["R"], 0, 2)
    # without both switches
    ctx.juncbed_reset()
    ctx.juncbed_best_alignments(True)
    ctx.juncbed_pair_alignments(True, *c["pair"])
    ctx.juncbed_add_pairs(L, R)
    ctx.juncbed_finish(8)
    with pytest.raises(host.ThjError, match=r"\(-5\).*not armed"):
        ctx.juncbed_report_pairs_bam(raw["L"], raw["R"])
    # the single-end switch beside graded inserts stays refused, in either order
    ctx.juncbed_reset()
    ctx.juncbed_best_alignments(True)
    ctx.juncbed_pair_alignments(True, *c["pair"])
    with pytest.raises(host.ThjError, match=r"\(-1\).*not built"):
        ctx.juncbed_collect_accepted(True, 1, "", [0, 1])
    ctx.juncbed_reset()
    ctx.juncbed_best_alignments(True)
    ctx.juncbed_collect_accepted(True, 1, "", [0, 1])
    with pytest.raises(host.ThjError, match=r"\(-1\).*not built"):
        ctx.juncbed_pair_alignments(True, *c["pair"])
    ctx.juncbed_reset()
    with pytest.raises(host.ThjError, match=r"\(-5\).*best alignments"):
        ctx.juncbed_collect_accepted(True, 1, "", [0, 1], pairs=True)
    # both, in either order; before the finish
    for first in (0, 1):
        ctx.juncbed_reset()
        ctx.juncbed_best_alignments(True)
        if first:
            ctx.juncbed_collect_accepted(True, 1, "", [0, 1], pairs=True)
        ctx.juncbed_pair_alignments(True, *c["pair"])
        if not first:
            ctx.juncbed_collect_accepted(True, 1, "", [0, 1], pairs=True)
        ctx.juncbed_add_pairs(L, R)
        with pytest.raises(host.ThjError, match=r"\(-5\).*thj_juncbed_finish first"):
            ctx.juncbed_report_pairs_bam(raw["L"], raw["R"])
        ctx.juncbed_finish(8)
        # the records of a side do not match the add call
        with pytest.raises(host.ThjError, match=r"\(-1\).*line up"):
            ctx.juncbed_report_pairs_bam(raw["L"], raw["R"][:2])
        with pytest.raises(host.ThjError, match=r"\(-1\).*line up"):
            ctx.juncbed_report_pairs_bam(raw["L"] + raw["L"][:1], raw["R"])
        want, _ = apr.accepted(c, raw, cfg)
        stream, sizes = ctx.juncbed_report_pairs_bam(raw["L"], raw["R"])
        assert stream == b"".join(want) and sizes == [len(w) for w in want]
        with pytest.raises(host.ThjError, match=r"\(-5\).*replayed already"):
            ctx.juncbed_report_pairs_bam(raw["L"], raw["R"])
    # a finish again: the replay starts over
    ctx.juncbed_finish(8)
    assert ctx.juncbed_report_pairs_bam(raw["L"], raw["R"])[0] == b"".join(want)
    # the single-end replay has nothing to replay here
    with pytest.raises(host.ThjError, match=r"\(-5\)"):
        ctx.juncbed_report_bam(write_bam(None, members_of(raw["L"], 2), targets=TARGETS).data, [1, 2], 500000)
    # a reset turns it off
    ctx.juncbed_reset()
    ctx.juncbed_best_alignments(True)
    ctx.juncbed_pair_alignments(True, *c["pair"])
    ctx.juncbed_add_pairs(L, R)
    ctx.juncbed_finish(8)
    with pytest.raises(host.ThjError, match=r"\(-5\).*not armed"):
        ctx.juncbed_report_pairs_bam(raw["L"], raw["R"])


def test_a_single_end_consensus_afterwards(ctx, crowd):
    """the same context: single-end accepted hits before and after a paired consensus are the same bytes, the restatement's"""
    sc = planted([1, 2, 16, 3], seed=12)
    raws = raw_records(sc)
    bam = [write_bam(None, members_of(raws, 7), targets=TARGETS).data]
    want, _seen = single_expected(sc, raws, single_cfg(2, "grp"), None)
    assert bc.GENOME == pc.GENOME                                # (the context's genome serves both)
    before = single_through_ctx(ctx, sc, bam, single_cfg(2, "grp"))
    c, raw = crowd
    check(ctx, c, raw, apc.cfg_of(2, "grp"))
    after = single_through_ctx(ctx, sc, bam, single_cfg(2, "grp"))
    assert before == after and before[0] == b"".join(want) and br.groups(sc["reads"])
