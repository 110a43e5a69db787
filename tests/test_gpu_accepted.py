"""GPU: accepted_hits.bam's records on the device (thj_juncbed_collect_accepted / thj_juncbed_report_bam, thj_junctions
--accepted-hits-out) against the restatement (accepted_ref.py on top of best_ref.py's choice): reads of the sizes at which the kernels
take another path (1, 2, 16 | 17, 20 on the host's std::sort list | 21 through the trim), a tie beyond 16 entries ordered by a std::sort
that tests/acceptedsim runs, read runs across wave, workgroup and grid-stride edges, runs held back across pieces, records that shrink
and grow, member cuts, --suppress-hits, two inputs, the contract, and the executable end to end."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import accepted_cases as ac
import accepted_ref as ar
import best_cases as bc
import best_ref as br
from ingest_cases import bam_header, bgzf_member, cw, record, tag, write_bam
from locked_make import locked_make
from test_gpu_binaries_reported import BAM_OP, EXE, members_of, write_ref
from tophat_amd import host

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["chrA", "chrB"]
TARGETS = tuple((n, len(s)) for n, s in zip(NAMES, bc.GENOME))
M, D = bc.M, bc.D
SIZES = [1, 2, 16, 17, 20, 21, 1, 3]


def aln(ref, left, dlen=2):
    return (ref, left, False, [(M, 20), (D, dlen), (M, 20)])


def planted(sizes, seed=3, tie_in=None, cap=20, suppress=False):
    """reads of the given numbers of candidates, all tied at AS 0 (so every candidate is reported, up to the cap), on both contigs in
    shuffled input order; tie_in: that read gets two alignments on one (contig, left) that differ in their deletion"""
    rng = np.random.default_rng(seed)
    reads_of = []
    for k, n in enumerate(sizes):
        spots = [(int(rng.integers(1, 3)), 200 + 50 * int(p)) for p in rng.permutation(60)[:n]]
        rd = [(aln(r, l), 0) for r, l in spots]
        if k == tie_in:
            rd[n // 2] = (aln(rd[2][0][0], rd[2][0][1], 3), 0)
        reads_of.append(rd)
    return bc.case("planted", reads_of, best=(cap, suppress, 6))


def raw_records(c, names=None):
    """the case's alignments as BAM records: tags of many kinds -- some shrink (an NM stored as i, a dropped NH, a dropped Z value),
    the appended ones grow"""
    out = []
    for k, r in enumerate(c["recs"]):
        nm = c["mism"][k] + sum(ln for op, ln in r[3] if op == D)
        aux = tag("NM", "i" if k % 3 == 0 else "C", nm) + tag("AS", "i" if k % 2 else "c", c["AS"][k])
        if k % 4 == 1:
            aux += tag("NH", "C", 7) + tag("ZW", "Z", "a value that held NH:i:3 " * 3)
        if k % 5 == 2:
            aux += tag("XS", "A", "+") + tag("YS", "s", -300) + tag("ZQ", "Z", "kept text")
        name = (names[k] if names else "q%d%s" % (c["reads"][k], "/1" if c["reads"][k] % 2 else ""))
        out.append(record(name, tid=r[0] - 1, pos=r[1], flag=0x10 if (k % 7 == 3 or c["anti"][k]) else 0, cigar=[cw(BAM_OP[op], ln) for op, ln in r[3]],
                          seq=[1 + (k + i) % 4 for i in range(40)], aux=aux))
    return out


def rec_key(rec):
    """(tid, pos, QNAME as it comes out) of a record with its block_size field"""
    tid, pos = struct.unpack_from("<ii", rec, 4)
    name = rec[36:36 + rec[12] - 1]
    return tid, pos, name[:-2] if name.endswith(b"/1") else name


def anti_of(raws):
    return [bool(struct.unpack_from("<H", r, 18)[0] & 0x10) for r in raws]


@pytest.fixture(scope="module")
def ctx():
    with host.Context(0) as c:
        c.upload_genome(host.pack_genome(bc.GENOME))
        c.bam_contig_names_upload(NAMES)
        yield c


@pytest.fixture(scope="module")
def order(tmp_path_factory):
    d = os.path.join(HERE, "acceptedsim")
    locked_make(d)
    tmp = tmp_path_factory.mktemp("order")

    def run(keys):
        p = tmp / "keys.txt"
        p.write_text("".join("%d %d\n" % k for k in keys))
        r = subprocess.run([os.path.join(d, "acceptedsim"), "order", str(p)], capture_output=True, text=True)
        assert r.returncode == 0
        return [int(x) for x in r.stdout.split()]
    return run


def cfg_of(library_type=1, rg=""):
    return {"library_type": library_type, "rg": rg, "names": NAMES, "header": NAMES}


def expected(c, raws, cfg, order):
    c = dict(c, anti=anti_of(raws))
    ch = br.choose(c["recs"], c["reads"], c["AS"], c["mism"], c["anti"], c["best"])
    return ar.accepted(c, ch, [r[4:] for r in raws], cfg, order)


def through_ctx(ctx, c, bams, cfg, per=None):
    """the whole call sequence -> (the stream, the record sizes)"""
    ctx.juncbed_reset()
    ctx.juncbed_best_alignments(True, *c["best"])
    ctx.juncbed_collect_accepted(True, cfg["library_type"], cfg["rg"], [0, 1])
    for b in bams:
        ctx.juncbed_add_bam(b, [1, 2], 500000, piece_members=per)
    ctx.juncbed_finish(8)
    sizes, total = [], 0
    for b in bams:
        s, total = ctx.juncbed_report_bam(b, [1, 2], 500000, piece_members=per)
        sizes += s
    return ctx.bam_stream_download(total), sizes


def check(ctx, c, raws, cfg, order, per_member=7, per=None, tmp_path=None, two=False):
    want, seen = expected(c, raws, cfg, order)
    if two:                                                    # two inputs, cut between two reads
        cut = br.groups(c["reads"])[len(set(c["reads"])) // 2][0]
        bams = [write_bam(None, members_of(raws[:cut], per_member), targets=TARGETS).data, write_bam(None, members_of(raws[cut:], per_member), targets=TARGETS).data]
    else:
        bams = [write_bam(None, members_of(raws, per_member), targets=TARGETS).data]
    stream, sizes = through_ctx(ctx, c, bams, cfg, per)
    assert sizes == [len(w) for w in want]
    assert stream == b"".join(want)
    return want, seen


def test_read_sizes_and_the_sort_list(ctx, order):
    """1, 2 and 16 are ordered by counting on the device; 17 and 20 reach the host's std::sort; 21 is trimmed to 20 first, then sorted there"""
    c = planted(SIZES)
    raws = raw_records(c)
    want, seen = check(ctx, c, raws, cfg_of(2, "grp"), order)
    assert seen == {"big": 3, "over": 1} and len(want) == sum(SIZES) - 1
    # records that shrink and records that grow
    len_in = {rec_key(r): len(r) for r in raws}
    change = [len(w) - len_in[rec_key(w)] for w in want]
    assert min(change) < -50 and max(change) > 10
    # the same through pieces of four members: runs are held back across piece boundaries (more_follows and the resume point)
    held = [s for s, e in br.groups(c["reads"]) if any(s < 28 * k < e for k in range(1, 4))]
    assert held
    check(ctx, c, raws, cfg_of(2, "grp"), order, per=4)
    check(ctx, c, raws, cfg_of(3), order, per=4, two=True)


def test_a_tie_beyond_16(ctx, order):
    """17 reported alignments, two of them on one (contig, left): the expected order is std::sort's own, run by tests/acceptedsim"""
    c = planted([2, 17, 1], seed=9, tie_in=1)
    raws = raw_records(c)
    ch = br.choose(c["recs"], c["reads"], c["AS"], c["mism"], anti_of(raws), c["best"])
    kept = sorted((i for i in range(2, 19) if ch["keep"][i]), key=lambda i: ch["rank"][i])
    keys = [(c["recs"][i][0], c["recs"][i][1]) for i in kept]
    assert len(kept) == 17 and len(set(keys)) == 16
    want, seen = check(ctx, c, raws, cfg_of(), order)
    assert seen["big"] == 1
    got_order = [struct.unpack_from("<ii", w, 4) for w in want[2:19]]
    assert got_order == [(keys[k][0] - 1, keys[k][1]) for k in order(keys)]


def test_suppress_hits(ctx, order):
    c = planted(SIZES, cap=16, suppress=True)
    want, seen = check(ctx, c, raw_records(c), cfg_of(), order)
    assert seen == {"big": 0, "over": 3} and len(want) == 1 + 2 + 16 + 1 + 3


def test_runs_across_wave_workgroup_and_stride_edges(ctx, order):
    """single-alignment reads fill up to the edges; reads of 5 lie across record 64, 256 and 32768 (the write kernel's wave stride:
    8192 workgroups of four waves)"""
    sizes = [1] * 62 + [5] + [1] * 187 + [5] + [1] * (32768 - 259 - 2) + [5] + [1] * 3
    starts = np.cumsum([0] + sizes)
    assert all(any(starts[k] < e < starts[k + 1] for k in range(len(sizes)) if sizes[k] == 5) for e in (64, 256, 32768))
    reads_of = [[(aln(1 + (k + j) % 2, 200 + 40 * ((7 * k + 3 * j) % 50) + j), 0) for j in range(n)] for k, n in enumerate(sizes)]
    c = bc.case("edges", reads_of)
    # records by the thousand: two alternating names tell the reads apart, the bytes are made once per shape
    raws, cache = [], {}
    for k, r in enumerate(c["recs"]):
        key = (c["reads"][k] % 2, r[0], r[1])
        if key not in cache:
            cache[key] = record("ab"[key[0]], tid=r[0] - 1, pos=r[1], cigar=[cw(BAM_OP[op], ln) for op, ln in r[3]], seq=[1] * 40, aux=tag("NM", "C", 2) + tag("AS", "C", 0))
        raws.append(cache[key])
    want, seen = check(ctx, c, raws, cfg_of(), order, per_member=500)
    assert len(want) == len(raws)


def test_a_read_across_the_grid_stride(ctx, order):
    """the per-record kernels run 4096 workgroups of 256 threads: a read of 5 lies across record 1048576.  The reads before it are
    single alignments of two alternating names: their rewritten records are worked out once"""
    n_fill = 1048574
    fill = [record("ab"[k], tid=0, pos=300, cigar=[cw(0, 40)], seq=[1] * 40, aux=tag("NM", "C", 0) + tag("AS", "C", 0)) for k in range(2)]
    big = [aln(1, 1000 + 40 * j) for j in range(5)]
    tail = planted([5, 2], seed=4)
    braw = [record("big", tid=0, pos=r[1], cigar=[cw(BAM_OP[op], ln) for op, ln in r[3]], seq=[2] * 40, aux=tag("NM", "C", 2) + tag("AS", "C", 0)) for r in big]
    traw = raw_records(tail)
    per = 500                                                   # fillers a member; the one member's bytes are made once and repeated
    one = bgzf_member(b"".join(fill[k % 2] for k in range(per)))
    n_members, rest = divmod(n_fill, per)
    data = bgzf_member(bam_header(TARGETS)) + one * n_members + bgzf_member(b"".join(fill[k % 2] for k in range(rest)) + b"".join(braw)) + \
        bgzf_member(b"".join(traw)) + bgzf_member(b"")
    assert n_members * per + rest == n_fill and n_fill < 4096 * 256 < n_fill + 5
    cfg = cfg_of()
    g = br.Mt19937(1)
    for _ in range(n_fill):
        g()
    out_fill = [ar.print_sam_for_single([(1, 0, f[4:])], 0, cfg)[0] for f in fill]
    want = [ar.print_sam_for_single([(1, 0, r[4:]) for r in braw], g(), cfg)]
    tc = dict(tail, anti=anti_of(traw))
    ch = br.choose(tc["recs"], tc["reads"], tc["AS"], tc["mism"], tc["anti"], tc["best"])
    for s, e in br.groups(tc["reads"]):
        kept = sorted((i for i in range(s, e) if ch["keep"][i]), key=lambda i: ch["rank"][i])
        want.append(ar.print_sam_for_single([(tc["recs"][i][0], ch["score"][i], traw[i][4:]) for i in kept], g(), cfg))
    stream, sizes = through_ctx(ctx, tail, [data], cfg)
    head = len(out_fill[0]) * ((n_fill + 1) // 2) + len(out_fill[1]) * (n_fill // 2)
    assert len(sizes) == n_fill + 5 + 7 and stream[head:] == b"".join(b"".join(w) for w in want)
    assert stream[:len(out_fill[0]) + len(out_fill[1])] == out_fill[0] + out_fill[1] and stream[head - len(out_fill[1]):head] == out_fill[1]


def padded(k, pad):
    return record("p%d" % k, tid=0, pos=300 + k, cigar=[cw(0, 40)], seq=[1] * 40, aux=tag("NM", "C", 0) + tag("AS", "C", 0) + tag("ZZ", "Z", "x" * pad))


def cut_case():
    """eight single-alignment reads of about 20 kB: record 3 ends exactly on byte 65536, record 6 is one byte too long for what is left
    of the second member"""
    pads = [20000] * 8
    cfg = cfg_of()
    size = lambda k: len(ar.print_sam_for_single([(1, 0, padded(k, pads[k])[4:])], 0, cfg)[0])      # noqa: E731
    pads[3] += 65536 - sum(size(k) for k in range(4))
    pads[6] += 65537 - sum(size(k) for k in range(4, 7))
    raws = [padded(k, pads[k]) for k in range(8)]
    c = bc.case("cuts", [[((1, 300 + k, False, [(M, 40)]), 0)] for k in range(8)])
    return c, raws


def test_member_cuts_and_the_deflater(ctx, order):
    c, raws = cut_case()
    want, _seen = check(ctx, c, raws, cfg_of(), order, per_member=2)
    sizes = [len(w) for w in want]
    cuts = host.bgzf_plan_cuts(sizes)
    assert cuts[:3] == [65536, 65536 + sizes[4] + sizes[5], 65536 + sum(sizes[4:8])] and sum(sizes[:4]) == 65536 and sum(sizes[4:7]) == 65537
    comp, crc = ctx.bgzf_deflate(cuts)
    stream = b"".join(want)
    for k, e in enumerate(cuts):
        b = cuts[k - 1] if k else 0
        assert zlib.decompress(comp[k], -15) == stream[b:e] and crc[k] == zlib.crc32(stream[b:e]) & 0xFFFFFFFF


# ---------------------------------------------------------------- the contract

def one_read_bam(hits):
    return write_bam(None, members_of([struct.pack("<i", len(h[2])) + h[2] for h in hits], 1), targets=TARGETS + (("chrC", 5000),), header_alone=True).data


@pytest.mark.parametrize("lc", ac.loud_cases(), ids=[x[0] for x in ac.loud_cases()])
def test_loud_cases(ctx, lc):
    label, hits, names = lc
    bam = one_read_bam(hits)
    ctx.juncbed_reset()
    ctx.juncbed_best_alignments(True)
    ctx.juncbed_collect_accepted(True, 1, "", [0, 1] if label != "contig" else [-1, 0])
    ctx.juncbed_add_bam(bam, [1, 2, 1], 500000)
    ctx.juncbed_finish(8)
    with pytest.raises(host.ThjError, match=r"\(-1\)") as e:
        ctx.juncbed_report_bam(bam, [1, 2, 1], 500000)
    assert names in str(e.value)


def test_call_order(ctx, order):
    c = planted([3, 2, 4], seed=6)
    raws = raw_records(c)
    bam = write_bam(None, members_of(raws, 2), targets=TARGETS).data
    ctx.juncbed_reset()
    with pytest.raises(host.ThjError, match=r"\(-5\).*best alignments"):
        ctx.juncbed_collect_accepted(True, 1, "", [0, 1])
    ctx.juncbed_best_alignments(True)
    with pytest.raises(host.ThjError, match=r"\(-1\)"):
        ctx.juncbed_collect_accepted(True, 1, "", [0])
    with pytest.raises(host.ThjError, match=r"\(-5\).*not armed"):
        ctx.juncbed_report_bam(bam, [1, 2], 500000)
    ctx.juncbed_collect_accepted(True, 1, "", [0, 1])
    ctx.juncbed_add_bam(bam, [1, 2], 500000)
    with pytest.raises(host.ThjError, match=r"\(-5\).*records were added already"):
        ctx.juncbed_collect_accepted(True, 1, "", [0, 1])
    with pytest.raises(host.ThjError, match=r"\(-5\).*thj_juncbed_finish first"):
        ctx.juncbed_report_bam(bam, [1, 2], 500000)
    ctx.juncbed_finish(8)
    # a piece of another record count
    fewer = write_bam(None, members_of(raws[:5], 2), targets=TARGETS).data
    with pytest.raises(host.ThjError, match=r"\(-1\).*line up"):
        ctx.juncbed_report_bam(fewer, [1, 2], 500000)
    # a piece of as many records whose read runs differ: 2, 3, 4 where 3, 2, 4 were added
    names = ["x%d" % k for k in (0, 0, 1, 1, 1, 2, 2, 2, 2)]
    other = write_bam(None, members_of(raw_records(c, names), 2), targets=TARGETS).data
    with pytest.raises(host.ThjError, match=r"\(-1\).*line up"):
        ctx.juncbed_report_bam(other, [1, 2], 500000)
    # the right piece, then one call too many
    sizes, total = ctx.juncbed_report_bam(bam, [1, 2], 500000)
    want, _ = expected(c, raws, cfg_of(), order)
    assert ctx.bam_stream_download(total) == b"".join(want) and sizes == [len(w) for w in want]
    with pytest.raises(host.ThjError, match=r"\(-5\).*replayed already"):
        ctx.juncbed_report_bam(bam, [1, 2], 500000)
    # records added by another call cannot be replayed
    ctx.juncbed_reset()
    ctx.juncbed_best_alignments(True)
    ctx.juncbed_collect_accepted(True, 1, "", [0, 1])
    a = host.aln_array_from_tuples(c["recs"][:3])
    ctx.juncbed_add_records(a)
    ctx.juncbed_finish(8)
    with pytest.raises(host.ThjError, match=r"\(-5\).*other calls"):
        ctx.juncbed_report_bam(bam, [1, 2], 500000)
    # a reset turns it off
    ctx.juncbed_reset()
    ctx.juncbed_best_alignments(True)
    ctx.juncbed_add_bam(bam, [1, 2], 500000)
    ctx.juncbed_finish(8)
    with pytest.raises(host.ThjError, match=r"\(-5\).*not armed"):
        ctx.juncbed_report_bam(bam, [1, 2], 500000)


# ---------------------------------------------------------------- the executable

def run_exe(tmp_path, tag_, ref_fa, hdr, bams, extra, env=None, ok=True):
    d = tmp_path / tag_
    d.mkdir()
    args = [EXE, "--insertions-out", str(d / "insertions.bed"), "--deletions-out", str(d / "deletions.bed")] + (["--sam-header", str(hdr)] if hdr else []) + extra
    r = subprocess.run(args + [str(ref_fa), str(d / "junctions.bed"), ",".join(str(b) for b in bams)], capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=120)
    if not ok:
        return r
    assert r.returncode == 0, (tag_, r.stderr[-1000:])
    return {f: open(d / f, "rb").read() for f in ("junctions.bed", "insertions.bed", "deletions.bed")}, r.stderr, d


def members(data):
    """-> [(inflated bytes, CRC-32 field, ISIZE field)]"""
    offs = host.bam_layout(data)[0]
    out = []
    for a, b in zip(offs, offs[1:]):
        xl = struct.unpack_from("<H", data, a + 10)[0]
        crc, isz = struct.unpack_from("<II", data, b - 8)
        out.append((zlib.decompress(data[a + 12 + xl:b - 8], -15), crc, isz))
    return out


def test_thj_junctions_accepted_hits_out(tmp_path, order):
    c, raws = cut_case()
    c2 = planted(SIZES, seed=8)
    raws2 = raw_records(c2)
    ref_fa, hdr = write_ref(tmp_path, NAMES, bc.GENOME)
    b1 = write_bam(str(tmp_path / "one.bam"), members_of(raws, 2), targets=TARGETS).path
    b2 = write_bam(str(tmp_path / "two.bam"), members_of(raws2, 7), targets=TARGETS).path
    cfg = cfg_of(2, "grp")
    # the generator runs on over both inputs: the expectation is made over their concatenation
    both = dict(c, recs=c["recs"] + c2["recs"], reads=c["reads"] + [r + 8 for r in c2["reads"]], AS=c["AS"] + c2["AS"], mism=c["mism"] + c2["mism"], anti=c["anti"] + c2["anti"])
    want, seen = expected(both, raws + raws2, cfg, order)
    assert seen == {"big": 3, "over": 1}
    opts = ["--best-alignments", "--library-type", "fr-firststrand", "--rg-id", "grp"]
    plain, _err, _d = run_exe(tmp_path, "plain", ref_fa, hdr, [b1, b2], opts, {"THJ_DEVICE_INGEST": "1", "THJ_PIECE_MEMBERS": "4"})
    got, err, d = run_exe(tmp_path, "acc", ref_fa, hdr, [b1, b2], opts + ["--accepted-hits-out", str(tmp_path / "accepted_hits.bam")], {"THJ_PIECE_MEMBERS": "4"})
    assert got == plain and "parsed on the device" in err                     # the three bed files, byte for byte
    ms = members(open(tmp_path / "accepted_hits.bam", "rb").read())
    assert all(zlib.crc32(m[0]) & 0xFFFFFFFF == m[1] and len(m[0]) == m[2] for m in ms) and ms[-1][2] == 0
    header = bam_header(TARGETS, open(hdr).read())
    sizes = [len(w) for w in want]
    cuts = host.bgzf_plan_cuts(sizes)
    assert [m[2] for m in ms] == [len(header)] + [e - (cuts[k - 1] if k else 0) for k, e in enumerate(cuts)] + [0]
    assert ms[0][0] == header and b"".join(m[0] for m in ms[1:]) == b"".join(want)
    assert "accepted hits: %d records" % len(want) in err and not os.path.exists(str(tmp_path / "accepted_hits.bam") + ".index")


def test_thj_junctions_refusals(tmp_path):
    c = planted([2, 3], seed=2)
    raws = raw_records(c)
    ref_fa, hdr = write_ref(tmp_path, NAMES, bc.GENOME)
    bam = write_bam(str(tmp_path / "in.bam"), members_of(raws, 2), targets=TARGETS).path
    out = ["--accepted-hits-out", str(tmp_path / "a.bam")]
    r = run_exe(tmp_path, "nobest", ref_fa, hdr, [bam], out, ok=False)
    assert r.returncode != 0 and "needs --best-alignments" in r.stderr
    r = run_exe(tmp_path, "nohdr", ref_fa, None, [bam], out + ["--best-alignments"], ok=False)
    assert r.returncode != 0 and "needs --sam-header" in r.stderr
    needs = "accepted hits need BAM inputs of whole BGZF members"
    r = run_exe(tmp_path, "host", ref_fa, hdr, [bam], out + ["--best-alignments"], {"THJ_HOST_INGEST": "1"}, ok=False)
    assert r.returncode != 0 and needs in r.stderr
    # records that straddle members: the add call declines the input
    whole = b"".join(raws)
    cut = len(raws[0]) + 30
    straddle = write_bam(str(tmp_path / "straddle.bam"), [([whole[:cut]], 6), ([whole[cut:]], 6)], targets=TARGETS).path
    r = run_exe(tmp_path, "straddle", ref_fa, hdr, [straddle], out + ["--best-alignments"], ok=False)
    assert r.returncode != 0 and needs in r.stderr
    # a loud record ends the run with its case's name
    bad = list(raws)
    bad[1] = bad[1][:4 + 14] + struct.pack("<H", 1) + bad[1][4 + 16:]
    badbam = write_bam(str(tmp_path / "paired.bam"), members_of(bad, 2), targets=TARGETS).path
    r = run_exe(tmp_path, "paired", ref_fa, hdr, [badbam], out + ["--best-alignments"], ok=False)
    assert r.returncode != 0 and "paired records: not built" in r.stderr
