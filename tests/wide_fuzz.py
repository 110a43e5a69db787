"""Adversarial batches at the wide shapes -- reads of up to 16 segments and 512 bases -- shared by test_fuzz_wide_cpu.py (kernel logic
against the oracle) and test_gpu_fuzz_wide.py (the real kernels against the oracle).

GRID covers the four instance choices of both stages, nseg <= 8 / nseg > 8 by W <= 4 / W > 4 (W: 64-bit words a bit plane), with read
lengths on both sides of every plane-word boundary, segment lengths 8..19 and 64, and last segments up to 2L - 1 bases long.  The batches
keep test_fuzz_cpu's content (hits at contig ends, tiny contigs, N runs in genome and read, antisense, spliced / deletion / insertion
segment hits, decoys, random qualities) and add test_fusion_long_reads_cpu's true hits and chimeric reads, which at these lengths are the
only reads the oracle can join."""
import numpy as np

from test_fusion_long_reads_cpu import rand_long_span_batch
from test_fuzz_cpu import fusion_set_near_hits, rand_genome, rand_seg_batch, rand_span_batch  # noqa: F401 (re-exported)
from tophat_amd.batch import HIT_DTYPE, JUNC_DTYPE, SegBatch, SpanBatch
from tophat_amd.params import Params

# (read length, segment length): nseg = rl // L, the last segment takes the rest
GRID = [
    # nseg <= 8, W <= 4: thj_k_fusion, thj_k_stitch_fusion, the packed tier
    (256, 32), (255, 64), (150, 18),
    # nseg > 8, W <= 4: thj_k_sj_flat<16> / thj_k_sj_general, thj_k_fusion, thj_k_stitch_fusion_wide
    (128, 8), (135, 8), (200, 13), (250, 25), (256, 16),
    # nseg <= 8, W > 4: thj_k_fusion_wide, thj_k_stitch_fusion_wide
    (257, 32), (321, 64), (385, 64), (449, 64), (511, 64), (512, 64),
    # nseg > 8, W > 4: both wide instances
    (257, 16), (274, 25), (320, 20), (321, 20), (384, 24), (448, 28), (449, 28), (511, 31), (512, 32),
]


def words(rl):
    return (rl + 63) // 64


def quadrant(rl, L):
    return (rl // L > 8, words(rl) > 4)


def shape_id(shape):
    rl, L = shape
    return "rl%d_L%d_n%d_W%d" % (rl, L, rl // L, words(rl))


def big_contig(rng, n):
    """a contig that holds any read: random bases with splice motifs, so that windows fire"""
    s = rng.choice(list("ACGT"), size=n)
    for _k in range(n // 40):
        p = int(rng.integers(0, n - 2))
        s[p:p + 2] = list(rng.choice(["GT", "AG", "GC", "AT", "AC", "CT"]))
    return "".join(s)


def genome(rng, n_small):
    seqs = rand_genome(rng, n_small)
    seqs.append(big_contig(rng, 6000))
    return seqs


def concat_span(a, b):
    """two SpanBatches of one nseg as one"""
    n = a.n_reads + b.n_reads
    return SpanBatch(a.nseg, np.arange(1, n + 1, dtype=np.uint32),
                     np.concatenate([a.read_off, b.read_off[1:] + a.read_off[-1]]).astype(np.int64),
                     np.concatenate([a.bases, b.bases]), np.concatenate([a.quals, b.quals]),
                     np.concatenate([a.seg_off, b.seg_off[1:] + a.seg_off[-1]]).astype(np.uint32), np.concatenate([a.hits, b.hits]))


def seg_with_true_hits(a, sb):
    """SegBatch a followed by the reads of SpanBatch sb (plain segment hits, no mates)"""
    h = sb.hits
    ln = (h["cigar"][:, 0] & 0x0FFFFFFF).astype(np.int64)
    t = np.zeros(len(h), dtype=HIT_DTYPE)
    t["ref_id"], t["left"], t["right"] = h["ref_id"], h["left"], h["left"] + ln
    t["flags"], t["edit_dist"], t["mismatches"], t["read_len"] = h["flags"] & 3, h["edit_dist"], h["mismatches"], ln
    n = a.n_reads + sb.n_reads
    args = [a.nseg, np.arange(1, n + 1, dtype=np.uint32), np.concatenate([a.read_off, sb.read_off[1:] + a.read_off[-1]]).astype(np.int64),
            np.concatenate([a.bases, sb.bases]), np.concatenate([a.seg_off, sb.seg_off[1:] + a.seg_off[-1]]).astype(np.uint32),
            np.concatenate([a.hits, t])]
    if a.mate_off is not None:
        args += [np.concatenate([a.mate_off, np.full(sb.n_reads, a.mate_off[-1])]).astype(np.uint32), a.mate_hits]
    return SegBatch(*args)


def seg_case(seed, shape, n_reads):
    """-> (contigs, SegBatch, Params): one stage-1 batch at `shape`, paired on odd seeds: test_fuzz_cpu's reads, then as many true-hit reads
    (half of them chimeric) without mates"""
    rl, L = shape
    nseg = rl // L
    rng = np.random.default_rng(31000 + seed)
    seqs = genome(rng, int(rng.integers(1, 4)))
    paired = bool(seed % 2)
    b = rand_seg_batch(rng, seqs, n_reads // 2, L, nseg, paired, rl=rl)
    if nseg > 1:
        b = seg_with_true_hits(b, rand_long_span_batch(rng, seqs, n_reads - n_reads // 2, L, nseg, rl=rl, n_rate=0.005, ends=True))
    p = Params(segment_length=L, read_side=1 + seed % 2, library_type=int(rng.choice([0, 0, 1, 2, 3])),
               min_segment_intron=int(rng.choice([10, 50])), max_segment_intron=int(rng.choice([400, 5000, 500000])),
               max_insertion_length=int(rng.choice([1, 3, 6])), max_deletion_length=int(rng.choice([1, 3, 10])),
               inner_dist_mean=int(rng.choice([0, 30, 50])), inner_dist_std_dev=int(rng.choice([5, 20, 60])),
               segment_mismatches=int(rng.choice([0, 2, 3])), fusion_min_dist=int(rng.choice([50, 1000])),
               fusion_anchor_length=int(rng.choice([8, 10, 20])))
    return seqs, b, p


def span_sets(rng, sb):
    """junctions and insertions dense around the hits (every plausible gap between two consecutive hits, a base either way), as
    test_fuzz_long_spanning_reads builds them"""
    juncs, ins = set(), {}
    h = sb.hits
    for k in range(0, len(h) - 1):
        a, b_ = h[k], h[k + 1]
        if a["ref_id"] != b_["ref_id"]:
            continue
        ra = int(a["left"]) + sum(int(c & 0x0FFFFFFF) for c in a["cigar"][:a["n_cigar"]] if (c >> 28) in (1, 5, 11))
        for d in (-2, 0, 1):
            l_, r_ = ra - 1 + d, int(b_["left"]) + d
            if r_ > l_ + 1 and l_ >= 0:
                juncs.add((int(a["ref_id"]), l_, r_, int(rng.integers(0, 2))))
        if 0 < ra - int(b_["left"]) <= 3:
            ins[(int(a["ref_id"]), int(b_["left"]) + int(rng.integers(-1, 2)), ra - int(b_["left"]))] = \
                "".join(rng.choice(list("ACGT"), size=ra - int(b_["left"])))
    jl = sorted(juncs)
    ja = np.array(jl, dtype=JUNC_DTYPE) if jl else np.zeros(0, dtype=JUNC_DTYPE)
    il = [(k[0], k[1], v) for k, v in sorted(ins.items()) if k[1] >= 0]
    return ja, il


def span_case(seed, shape, n_reads):
    """-> (contigs, SpanBatch, Params, junctions, insertions, fusion list): one stage-2 batch at `shape`, half test_fuzz_cpu's random
    hits, half true hits (chimeric reads among them, N in the read, parts at contig ends) with decoys"""
    rl, L = shape
    nseg = rl // L
    rng = np.random.default_rng(37000 + seed)
    seqs = genome(rng, int(rng.integers(1, 3)))
    a = rand_span_batch(rng, seqs, n_reads // 2, L, nseg, rl=rl)
    b = rand_long_span_batch(rng, seqs, n_reads - n_reads // 2, L, nseg, rl=rl, n_rate=0.005, ends=True) if nseg > 1 else a
    sb = concat_span(a, b) if nseg > 1 else a
    p = Params(segment_length=L, max_insertion_length=int(rng.choice([1, 3])), max_deletion_length=int(rng.choice([1, 3, 10])),
               min_report_intron=int(rng.choice([10, 50])), max_report_intron=int(rng.choice([300, 5000, 500000])),
               read_mismatches=int(rng.choice([6, 10, 14])), read_edit_dist=int(rng.choice([8, 12, 16])),
               read_gap_length=int(rng.choice([2, 3])))
    p.fusion_min_dist = int(rng.choice([100, 1500]))
    ja, il = span_sets(rng, sb)
    return seqs, sb, p, ja, il, fusion_set_near_hits(rng, sb)


def short_exon_case(seed=3, n_reads=120, L=16, nseg=16):
    """reads of nseg x L bases (+ up to L - 1) from a gene of 17..60-base exons: every segment hit is the true one, spliced (aM gN bM, or
    two junctions) where it crosses an exon end, and the junction set holds every intron -- joined alignments of 11 to 25 CIGAR ops.
    -> (contigs, SpanBatch, junctions)"""
    from tophat_amd.batch import SPAN_HIT_DTYPE
    rng = np.random.default_rng(41000 + seed)
    g, exons, pos = list(rng.choice(list("ACGT"), size=200)), [], 200
    while pos < 30000:
        e = int(rng.integers(17, 61))
        exons.append((pos, e))
        g += list(rng.choice(list("ACGT"), size=e))
        intr = int(rng.integers(60, 150))
        g += ["G", "T"] + list(rng.choice(list("ACGT"), size=intr - 4)) + ["A", "G"]
        pos += e + intr
    seq = "".join(g) + "".join(rng.choice(list("ACGT"), size=200))
    tmap = np.concatenate([np.arange(p, p + e) for p, e in exons])             # transcript base -> genome position
    juncs = np.array([(1, p + e - 1, exons[k + 1][0], 0) for k, (p, e) in enumerate(exons[:-1])], dtype=JUNC_DTYPE)
    hits, seg_off, bases, quals, read_off = [], [0], bytearray(), bytearray(), [0]
    for _r in range(n_reads):
        rl = nseg * L + int(rng.integers(0, L))
        t0 = int(rng.integers(0, len(tmap) - rl))
        for s in range(nseg):
            x = t0 + s * L
            ln = L if s < nseg - 1 else t0 + rl - x
            gp = tmap[x:x + ln]
            cig, run = [], 1
            for k in range(1, ln + 1):
                if k == ln or gp[k] != gp[k - 1] + 1:
                    cig.append((1 << 28) | run)
                    if k < ln:
                        cig.append((11 << 28) | int(gp[k] - gp[k - 1] - 1))
                    run = 1
                else:
                    run += 1
            hits.append((1, int(gp[0]), 2 if s == nseg - 1 else 0, 0, 0, len(cig), cig + [0] * (5 - len(cig))))
            seg_off.append(len(hits))
        bases += "".join(seq[i] for i in tmap[t0:t0 + rl]).encode()
        quals += bytes(int(q) for q in rng.integers(33, 75, size=rl))
        read_off.append(len(bases))
    sb = SpanBatch(nseg, np.arange(1, n_reads + 1, dtype=np.uint32), np.array(read_off, dtype=np.int64),
                   np.frombuffer(bytes(bases), dtype=np.uint8).copy(), np.frombuffer(bytes(quals), dtype=np.uint8).copy(),
                   np.array(seg_off, dtype=np.uint32), np.array(hits, dtype=SPAN_HIT_DTYPE))
    return [seq], sb, juncs


def n_ops(a):
    return sum(1 for c in a.cigar if c)
