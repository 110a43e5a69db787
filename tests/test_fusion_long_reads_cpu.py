"""CPU: --fusion-search on reads of more than eight segments or 256 bases (up to 16 and 512) -- both stages' kernel logic
(thj_core.h's fusion_eval with eight mask words, thj_fusion_block.h's workgroup, thj_span_fusion.h's 16-segment instance) against
the plain-C oracle.  The stage-2 oracle holds reads of up to 512 bases (spanning_fusion_oracle.c: MAXSEQ), the device limit; the
longest shapes are also checked by their properties."""
import functools

import numpy as np
import pytest

import orc
import sim
from bench import sample_segbatch, sample_spanbatch
from tophat_amd.batch import build_seg_batch, events_to_span_inputs, merge_events
from tophat_amd.params import Params
from tophat_amd.synth import make_case, make_device_workload, make_scale_genome

# (read length, segment length): 10, 15, 16, 16 and 15 segments; 4, 5, 5, 7 and 8 plane words
SHAPES = [(250, 25), (300, 20), (320, 20), (400, 25), (480, 32)]
ORACLE_MAXSEQ = 512

OP_FUS = (7, 8, 9, 10)


def fusion_list_from_events(f):
    rows = sorted({(int(x["ref_id1"]), int(x["ref_id2"]), int(x["left"]), int(x["right"]), int(x["dir"])) for x in f})
    return np.array(rows, dtype=orc.SPAN_FUSION_DTYPE) if rows else np.zeros(0, dtype=orc.SPAN_FUSION_DTYPE)


@functools.lru_cache(maxsize=None)
def genome():
    seqs, genes = make_scale_genome(1, [2_000_000, 1_000_000], 1500, intron_max=4000, exon_len=600)
    return seqs, genes, [s.tobytes().decode() for s in seqs]


@functools.lru_cache(maxsize=None)
def workload(rl, L, n=2000, seed=7):
    """make_device_workload's chimeric-left-read shape at read length rl, segment length L -> (genome strings, workload, n, chimeric rows,
    [(Params, SegBatch)] of both sides, the stage-1 oracle fusions of both sides)"""
    seqs, genes, strs = genome()
    w = make_device_workload(seed, seqs, genes, None, n, "cpu", exon_len=600, read_len=rl, seg_len=L, fusion_frac=0.04)
    fz = frozenset(w["left"]["fusion_reads"].tolist())
    og = orc.Genome(strs)
    sides, fus, ev = [], None, None
    for sd, side in (("left", 1), ("right", 2)):
        p = Params(read_side=side, segment_length=L, inner_dist_mean=50, inner_dist_std_dev=20, fusion_min_dist=100000)
        sb = sample_segbatch(w[sd], n)
        f = orc.fusions(p, og, sb, p.fusion_anchor_length, p.fusion_min_dist)
        e = orc.segjuncs(p, og, sb)
        ev = e if ev is None else merge_events(ev, e)
        fus = f if fus is None else orc.merge_fusions(fus, f)
        sides.append((p, sb, f))
    return strs, w, n, fz, sides, fus, ev


# ---- stage 1: find_fusions + detect_fusion

@pytest.mark.parametrize("rl,L", SHAPES, ids=lambda v: str(v))
def test_stage1_scale_workload_matches_oracle(rl, L):
    strs, w, n, fz, sides, fus, _ = workload(rl, L)
    assert sides[0][1].nseg == -(-rl // L)
    for p, sb, want in sides:
        assert sim.fusions(p, strs, sb).tolist() == want.tolist()
        got, _ = sim.fusions_block(p, strs, sb, 2)
        assert got.tolist() == want.tolist()
    assert len(fus) > 0.8 * len(fz) > 40


@pytest.mark.parametrize("rl,L", SHAPES, ids=lambda v: str(v))
def test_stage1_paired_case_matches_oracle(rl, L):
    case = make_case(seed=rl, paired=True, read_len=rl, seg_len=L, n_reads=300, fusion_reads=120, contig_lens=(60000, 50000, 40000),
                     exon_range=(300, 700))
    seqs = [orc.fold_genome_char(s) for s in case.seqs]
    g = orc.Genome(seqs)
    total = 0
    for sd, side in (("left", 1), ("right", 2)):
        other = "right" if sd == "left" else "left"
        b = build_seg_batch(case.seg_recs[sd], case.reads[sd], case.full_recs[other], case.seg_recs[other][-1], include_top0=True)
        p = Params(read_side=side, segment_length=L, fusion_min_dist=1000, inner_dist_mean=50, inner_dist_std_dev=20)
        want = orc.fusions(p, g, b, p.fusion_anchor_length, p.fusion_min_dist)
        assert sim.fusions(p, seqs, b).tolist() == want.tolist()
        assert sim.fusions_block(p, seqs, b, 1)[0].tolist() == want.tolist()
        total += len(want)
    assert total > 20


# ---- stage 2: the fusion tier of long_spanning_reads

def stage2_inputs(rl, L):
    strs, w, n, fz, sides, fus, ev = workload(rl, L)
    juncs, ins = events_to_span_inputs(ev)
    return strs, n, fz, juncs, ins, fusion_list_from_events(fus), sample_spanbatch(w["left"], n), sides[0][0].segment_length


@pytest.mark.parametrize("variant", ["tier0", "skip_tier0", "wave"])
@pytest.mark.parametrize("rl,L", SHAPES[:3], ids=lambda v: str(v))       # (400 and 480 bases: test_stage2_long_reads_by_properties)
def test_stage2_matches_oracle(rl, L, variant, monkeypatch):
    strs, n, fz, juncs, ins, fl, spb, _ = stage2_inputs(rl, L)
    og = orc.Genome(strs)
    p = Params(fusion_search=1, fusion_min_dist=100000, segment_length=L)
    want = orc.spanning_fusion(p, og, spb, juncs, ins, fl, True)
    if variant == "wave":
        monkeypatch.setenv("THJ_HOSTSIM_FUSWAVE", "4096")
    got, status = sim.spanning_fusion(p, strs, spb, juncs, ins, fl, skip_tier0=variant == "skip_tier0")
    assert status[1] == 0 and status[2] == 0
    assert got == want
    joined = {a.read_idx for a in want if a.is_fusion()}
    assert joined <= fz and len(joined) >= 0.8 * len(fz)
    plain = orc.spanning(Params(segment_length=L), og, spb, juncs, ins)
    assert [a for a in want if a.read_idx not in fz] == [a for a in plain if a.read_idx not in fz]


def _comp(s):
    return s.translate(str.maketrans("ACGTN", "TGCAN"))[::-1]


def rebuild(a, strs):
    """the sequence an alignment describes, from the genome: the pieces of both contigs its CIGAR walks (M up the genome, m down it,
    reverse-complemented; N / n / D / d skip)"""
    ref, pos, out = a.ref_id, a.left, []
    for c in a.cigar:
        op, ln = c >> 28, c & 0x0FFFFFFF
        if op in OP_FUS:
            ref, pos = a.ref_id2, ln
        elif op == 1:                                 # M
            out.append(strs[ref - 1][pos:pos + ln]); pos += ln
        elif op == 2:                                 # m
            out.append(_comp(strs[ref - 1][pos - ln + 1:pos + 1])); pos -= ln
        elif op in (5, 11):
            pos += ln
        elif op in (6, 12):
            pos -= ln
        else:
            raise AssertionError("op %d in a fusion alignment of this workload" % op)
    return "".join(out)


def md_of(ref, seq):
    """the MD string of an ungapped alignment of seq against ref"""
    out, run = [], 0
    for r_, q in zip(ref, seq):
        if r_ == q:
            run += 1
        else:
            out.append("%d%s" % (run, r_)); run = 0
    return "".join(out) + str(run)


def break_key(a):
    """the fusion an alignment goes through (fusions.cpp:441-495: the position walked up to the fusion op, one base back for fr / ff, one
    on for rf / rr; the op's length is the position on the second contig)"""
    pos = a.left
    for c in a.cigar:
        op, ln = c >> 28, c & 0x0FFFFFFF
        if op in (1, 5, 11):
            pos += ln
        elif op in (2, 6, 12):
            pos -= ln
        elif op in OP_FUS:
            pos = pos + 1 if op in (9, 10) else pos - 1
            return (a.ref_id, a.ref_id2, pos & 0xFFFFFFFF, ln, op)
    return None


@pytest.mark.parametrize("rl,L", SHAPES[3:], ids=lambda v: str(v))
def test_stage2_long_reads_by_properties(rl, L, monkeypatch):
    """400 and 480 bases: the oracle's records; besides, the non-chimeric reads come out as the plain path gives them; every fusion alignment
    has one fusion op, a second contig, a CIGAR that spans the read, rebuilds the read from the genome with its NM, and breaks at a stage-1
    fusion"""
    strs, n, fz, juncs, ins, fl, spb, _ = stage2_inputs(rl, L)
    og = orc.Genome(strs)
    p = Params(fusion_search=1, fusion_min_dist=100000, segment_length=L)
    got, status = sim.spanning_fusion(p, strs, spb, juncs, ins, fl)
    assert status[1] == 0 and status[2] == 0
    assert got == orc.spanning_fusion(p, og, spb, juncs, ins, fl, True)
    monkeypatch.setenv("THJ_HOSTSIM_FUSWAVE", "4096")
    assert sim.spanning_fusion(p, strs, spb, juncs, ins, fl, skip_tier0=True)[0] == got
    plain = orc.spanning(Params(segment_length=L), og, spb, juncs, ins)
    assert len(plain) > 0.1 * n
    assert [a for a in got if a.read_idx not in fz] == [a for a in plain if a.read_idx not in fz]
    keys = {tuple(int(v) for v in row) for row in fl.tolist()}
    fused = [a for a in got if a.is_fusion()]
    assert len(fused) > 0
    for a in fused:
        ops = [c >> 28 for c in a.cigar]
        assert sum(1 for o in ops if o in OP_FUS) == 1
        assert 1 <= a.ref_id2 <= len(strs)
        assert sum(c & 0x0FFFFFFF for c in a.cigar if (c >> 28) in (1, 2, 3, 4)) == rl
        # rebuilt from the genome it is the read (or its reverse complement) up to its mismatches, which NM and MD count
        bases, read = rebuild(a, strs), spb.bases[spb.read_off[a.read_idx]:spb.read_off[a.read_idx + 1]].tobytes().decode()
        assert len(bases) == rl
        seq = _comp(read) if a.antisense else read                    # the record's SEQ
        assert sum(1 for x, y in zip(bases, seq) if x != y) == a.mismatches == a.edit_dist == a.XM
        assert a.MD == md_of(bases, seq)
        # the break is one of stage 1's fusions: (contig, contig, left, right, direction) as fusions_from_spliced_hit takes it
        assert break_key(a) in keys
    joined = {a.read_idx for a in fused}
    assert joined <= fz and len(joined) >= 0.8 * len(fz)


# ---- the fusion tier on random batches of 9..16 segments (the fuzz of test_fuzz_cpu stops at eight).  rand_span_batch's hits are
# random in place and mismatch count, which at these lengths leaves the oracle nothing to join; here every segment has its true hit
# (its mismatches counted), the chimeric reads' second part comes from another locus in either orientation, and decoy hits lie around.

def rand_long_span_batch(rng, seqs, n_reads, L, nseg, rl=None, n_rate=0.0, ends=False):
    """rl: the read length (drawn when None); n_rate: the share of read bases turned into N (counted as mismatches of the true hits);
    ends: a true part starts at its contig's first or ends at its last base two times in three"""
    from test_fuzz_cpu import rand_hit
    from tophat_amd.batch import SPAN_HIT_DTYPE, SpanBatch
    rl = L * nseg + int(rng.integers(0, L)) if rl is None else rl
    comp = str.maketrans("ACGTN", "TGCAN")
    hits, seg_off, bases, quals, read_off = [], [0], bytearray(), bytearray(), [0]
    for _r in range(n_reads):
        brk = int(rng.integers(1, nseg)) * L if rng.random() < 0.5 else rl
        parts, read = [], ""
        for o, n in ((0, brk), (brk, rl - brk)):
            if n <= 0:
                continue
            ref = int(rng.integers(1, len(seqs) + 1))
            while len(seqs[ref - 1]) < n + 2:
                ref = int(rng.integers(1, len(seqs) + 1))
            pos, anti = int(rng.integers(0, len(seqs[ref - 1]) - n + 1)), int(rng.random() < 0.5)
            if ends:
                pos = int(rng.choice([0, len(seqs[ref - 1]) - n, pos]))
            t = seqs[ref - 1][pos:pos + n]
            parts.append((o, n, ref, pos, anti))
            read += t.translate(comp)[::-1] if anti else t
        read = "".join(c if rng.random() > 0.01 else rng.choice(list("ACGT")) for c in read)
        if n_rate:
            read = "".join(c if rng.random() > n_rate else "N" for c in read)
        for sg in range(nseg):
            x = sg * L
            ln = L if sg < nseg - 1 else rl - x
            o, n, ref, pos, anti = next(q for q in parts if q[0] <= x < q[0] + q[1])
            left = pos + (x - o) if not anti else pos + n - (x - o) - ln
            g = seqs[ref - 1][left:left + ln]
            piece = read[x:x + ln]
            if anti:
                g = g.translate(comp)[::-1]
            mm = sum(1 for u, v in zip(piece, g) if u != v or u == "N")
            end = 2 if sg == nseg - 1 else 0
            if mm <= 3:
                hits.append((ref, left, anti | end, mm, mm, 1, [(1 << 28) | ln, 0, 0, 0, 0]))
            for _ in range(int(rng.choice([0, 0, 0, 1, 2]))):
                dref, dleft = rand_hit(rng, seqs, L, (ref, left))
                dl = min(ln, len(seqs[dref - 1]) - dleft)
                if dl >= 1:
                    dmm = int(rng.integers(0, 3))
                    hits.append((dref, dleft, int(rng.integers(0, 2)) | end, dmm, dmm, 1, [(1 << 28) | dl, 0, 0, 0, 0]))
            seg_off.append(len(hits))
        bases += read.encode()
        quals += bytes(int(x) for x in rng.integers(33, 75, size=rl))
        read_off.append(len(bases))
    return SpanBatch(nseg, np.arange(1, n_reads + 1, dtype=np.uint32), np.array(read_off, dtype=np.int64),
                     np.frombuffer(bytes(bases), dtype=np.uint8).copy(), np.frombuffer(bytes(quals), dtype=np.uint8).copy(),
                     np.array(seg_off, dtype=np.uint32), np.array(hits, dtype=SPAN_HIT_DTYPE))


@pytest.mark.parametrize("seed", range(8))
def test_fuzz_fusion_tier_many_segments(seed):
    from test_fuzz_cpu import JUNC_DTYPE, fusion_set_near_hits, rand_genome
    rng = np.random.default_rng(9300 + seed)
    seqs = rand_genome(rng, int(rng.integers(2, 4)))
    seqs.append("".join(rng.choice(list("ACGT"), size=6000)))          # a contig that holds any read
    L = int(rng.choice([16, 18, 20, 32]))
    nseg = int(rng.integers(9, 17))
    if L * (nseg + 1) > ORACLE_MAXSEQ:
        nseg = ORACLE_MAXSEQ // L - 1
    sb = rand_long_span_batch(rng, seqs, 80, L, nseg)
    p = Params(segment_length=L, max_insertion_length=int(rng.choice([1, 3])), max_deletion_length=int(rng.choice([1, 3, 10])),
               min_report_intron=int(rng.choice([10, 50])), max_report_intron=int(rng.choice([300, 5000, 500000])),
               read_mismatches=int(rng.choice([6, 10])), read_edit_dist=int(rng.choice([8, 12])), read_gap_length=int(rng.choice([2, 3])))
    p.fusion_min_dist = int(rng.choice([100, 1500]))
    g = orc.Genome(seqs)
    fus = fusion_set_near_hits(rng, sb)
    ja = np.zeros(0, dtype=JUNC_DTYPE)
    for fs in (0, 1):
        p.fusion_search = fs
        want = orc.spanning_fusion(p, g, sb, ja, [], fus, bool(fs))
        assert len({a.read_idx for a in want}) > 10
        if fs:
            assert any(a.is_fusion() for a in want)
        for skip0 in (False, True):
            got, status = sim.spanning_fusion(p, seqs, sb, ja, [], fus, skip0)
            assert status[1] == 0
            got.sort(key=lambda a: a.read_idx)
            assert got == want, "seed %d fusion_search %d skip_tier0 %s" % (seed, fs, skip0)


# ---- a repeat family at more than eight segments: the workgroup's paths for reads with many hits (thj_fusion_block.h (a'), (b')) and
# the fusion tier's wave per read

@functools.lru_cache(maxsize=None)
def family_workload(rl, L, n=2400):
    """family_fusion_batches (test_hostsim_fusions) at read length rl, segment length L: a 41-copy family further apart than
    --fusion-min-dist, 2 % chimeric reads, and for every third read only the first segment mapped (its mate-anchored part runs over
    k x k (hit, mate hit) pairs).  -> (genome strings, [(Params, SegBatch)], reads with >= 64 (first, last) hit pairs, reads with >= 256
    (hit, mate hit, hit) triples, the workload)"""
    seqs, genes = make_scale_genome(1, [4_000_000], 3000, intron_max=1500, exon_len=600)
    S, copies = 40_000, 41
    for k in range(1, copies):
        seqs[0][k * S:(k + 1) * S] = seqs[0][:S]
    fam = genes[:, 3] + 600 + 1000 < S
    uniq = genes[:, 1] >= copies * S + 1000
    genes = genes[fam | uniq]
    strs = [s.tobytes().decode() for s in seqs]
    w = make_device_workload(9, seqs, genes, None, n, "cpu", exon_len=600, read_len=rl, seg_len=L, multi_frac=0.3, dup_shift=S,
                             max_copies=copies, fusion_frac=0.02)
    out, heavy_pairs, heavy_mates = [], 0, 0
    for sd, side in (("left", 1), ("right", 2)):
        p = Params(read_side=side, segment_length=L, inner_dist_mean=50, inner_dist_std_dev=20, fusion_min_dist=30000)
        sb = sample_segbatch(w[sd], n)
        so = sb.seg_off.astype(np.int64)
        keep = np.ones(len(sb.hits), dtype=bool)
        for r in range(0, n, 3):
            keep[so[r * sb.nseg + 1]:so[(r + 1) * sb.nseg]] = False
        cnt = np.array([int(keep[so[k]:so[k + 1]].sum()) for k in range(n * sb.nseg)], dtype=np.int64)
        sb.hits = sb.hits[keep]
        sb.seg_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
        cells = cnt.reshape(n, sb.nseg)
        heavy_pairs += int(((cells[:, 0] * cells[:, sb.nseg - 1]) >= 64).sum())
        heavy_mates += int((cells[0::3, 0] ** 2 * np.diff(sb.mate_off.astype(np.int64))[0::3] >= 256).sum())
        out.append((p, sb))
    return strs, out, heavy_pairs, heavy_mates, w


@pytest.mark.parametrize("rl,L", [(250, 25), (400, 25)], ids=lambda v: str(v))
def test_stage1_repeat_family_many_segments(rl, L):
    """10 segments / 4 words (thj_k_fusion) and 16 segments / 7 words (thj_k_fusion_wide): the family reads the workgroup takes together,
    same FusionSimpleSet as the oracle"""
    strs, batches, heavy_pairs, heavy_mates, _ = family_workload(rl, L)
    assert batches[0][1].nseg == -(-rl // L)
    assert heavy_pairs > 20 and heavy_mates > 20
    g = orc.Genome(strs)
    total = 0
    for p, sb in batches:
        want = orc.fusions(p, g, sb, p.fusion_anchor_length, p.fusion_min_dist)
        for n_blocks in (1, 3):
            assert sim.fusions_block(p, strs, sb, n_blocks)[0].tolist() == want.tolist()
        total += len(want)
    assert total > 50


def test_stage2_repeat_family_ten_segments(monkeypatch):
    """2 x 250 bp on the family: the fusion tier joins a family read's segments across copies -- a thread a read where the list fits, the
    wave a read (fusion_read_wave) for all -- as the oracle does"""
    strs, batches, _, _, w = family_workload(250, 25)
    g = orc.Genome(strs)
    fus = None
    for p, sb in batches:
        f = orc.fusions(p, g, sb, p.fusion_anchor_length, p.fusion_min_dist)
        fus = f if fus is None else orc.merge_fusions(fus, f)
    fl = fusion_list_from_events(fus)
    p = Params(fusion_search=1, segment_length=25, fusion_min_dist=30000)
    n = 600
    spb = sample_spanbatch(w["left"], n)
    want = orc.spanning_fusion(p, g, spb, _no_juncs(), [], fl, True)
    so = spb.seg_off.astype(np.int64).reshape(-1)
    heavy = sum(1 for r in range(n) if (so[r * 10 + 1] - so[r * 10]) * (so[r * 10 + 2] - so[r * 10 + 1]) >= 9)   # fusion_read_heavy: the wave's reads
    assert heavy > 20 and len(want) > n // 2 and any(a.is_fusion() for a in want)
    monkeypatch.setenv("THJ_HOSTSIM_FUSWAVE", "65536")
    got, status = sim.spanning_fusion(p, strs, spb, _no_juncs(), [], fl)
    assert status[1] == 0 and got == want


def _no_juncs():
    from tophat_amd.batch import JUNC_DTYPE
    return np.zeros(0, dtype=JUNC_DTYPE)
