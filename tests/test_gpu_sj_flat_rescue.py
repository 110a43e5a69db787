"""GPU: the mate-anchored rescue of stage 1's flat reads (thj_k_sj_flat lists them with a 32-byte entry each, thj_k_sj_rescue_flat scans
the flanks of their mate hits and enumerates, a thread a read) against the oracle -- junctions, deletions, insertions, `windows` and
`rescue_pairs`.  Planted reads: one hit a segment in the first `size` segments (abutting: no partner, so the read takes the rescue),
its last bases planted at a chosen distance from the first-segment hit, its mate hits laid so that their flanks hold that place.
Kinds: a pair that suits at size 2 and 3, sense and antisense; a mate hit on the other contig; on the same strand; a first mate
hit so close to the contig's start that the reference leaves its mate loop, with a good second one; a flank the contig's end cuts;
a pseudo-hit that abuts; one below min_segment_intron; one at max_segment_intron; two mate hits that both give windows.  Neighbours
that are not listed: no mate hit, three mate hits (the general rescue), no hit in the first segment.  The planted inputs are checked
on the CPU first: the oracle alone must show every kind's signature.  A workgroup's slice is what its tile of 256 consecutive reads
lists: tiles with 0, 1, 63, 64, 65, 255 and 256 listed reads, and (a batch of 2 048 tiles, all but two of them reads without a hit:
workgroup 0 takes the first and the last) 257, the slice's second round."""
import numpy as np
import pytest

import orc
from tophat_amd import host
from tophat_amd.batch import HIT_DTYPE, SegBatch
from tophat_amd.params import Params, READ_LEFT
from util import assert_events_equal

pytestmark = pytest.mark.gpu
L, CL = 25, 15
MEAN, SD = 50, 20          # the mate hit's flank: MEAN + SD bases
SPAN = 1500                # genome bases a read has to itself
CONTIG2 = 3000

#         kind: (antisense first hit, size, distance of the pseudo-hit from the first-segment hit)
SHAPE = {"ok2": (False, 2, 200), "ok3": (False, 3, 230), "anti2": (True, 2, 180), "anti3": (True, 3, 260), "contig": (False, 2, 200),
         "strand": (True, 2, 200), "break_good": (False, 2, 200), "clip": (True, 2, 200), "abut": (False, 2, 0), "near": (True, 2, 49),
         "far": (False, 2, 400), "two": (False, 3, 150), "m0": (False, 2, 200), "m3": (True, 2, 200), "nofirst": (False, 3, 230)}
LISTED = ("ok2", "ok3", "anti2", "anti3", "contig", "strand", "break_good", "clip", "abut", "near", "far", "two")
NEIGHBOURS = ("m0", "m3", "nofirst")
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def make_batch(kinds, nseg, seed=16, empty_between=None, drop_first_mate=False):
    """kinds[r] = the kind of read r; empty_between = (at, count): that many reads without a hit behind read `at`;
    drop_first_mate: the reads lose their first mate hit (the control of `break_good`)"""
    rng = np.random.default_rng(seed)
    rl = nseg * L
    g = rng.choice(list("ACGT"), size=2000 + SPAN * len(kinds))
    g2 = "".join(rng.choice(list("ACGT"), size=CONTIG2))
    clen = len(g)
    hits, seg_off, reads, mate_off, mate_hits = [], [0], [], [0], []
    for r, kind in enumerate(kinds):
        anti, size, dist = SHAPE[kind]
        size = min(size, nseg)
        B = 1000 + r * SPAN + 700
        cut = L if size <= 2 else L + 10         # the read leaves the first hit's stretch here: in segment 1 when the pseudo-hits stand in segment 2
        per_seg = [[] for _ in range(nseg)]
        if not anti:
            q = B + L + dist                     # where the read's last CL bases lie: the forward pseudo-hit's left
            J = q + CL - (rl - cut)
            if J - (B + cut) >= 20:
                g[B + cut:B + cut + 2] = list("GT")
                g[J - 2:J] = list("AG")
            seq = "".join(g[B:B + cut]) + "".join(g[J:J + rl - cut])
            for s in range(size):
                per_seg[s] = [(1, B + s * L, B + (s + 1) * L, 2 if s == nseg - 1 else 0, 0, 0, L)]
            over = [(1, q + CL + off, q + CL + off + 100, 1 | 2, 0, 0, 100) for off in (5, 16, 27)]        # antisense mate hits: q in [left - flank, left)
        else:
            q = B - dist - CL                    # the reverse pseudo-hit's left; it ends `dist` before the first hit
            E = q + (rl - cut)
            if (B + L - cut) - E >= 20:
                g[E:E + 2] = list("GT")
                g[B + L - cut - 2:B + L - cut] = list("AG")
            fwd = "".join(g[q:E]) + "".join(g[B + L - cut:B + L])
            seq = "".join(COMP[c] for c in reversed(fwd))
            for s in range(size):
                per_seg[s] = [(1, B - s * L, B - s * L + L, 1 | (2 if s == nseg - 1 else 0), 0, 0, L)]
            over = [(1, q - off - 100, q - off, 2, 0, 0, 100) for off in (5, 16, 27)]                      # sense mate hits: q in [right, right + flank)
        mates = over[:1]
        if kind == "contig":
            mates = [(2, 500, 600, over[0][3], 0, 0, 100)]
        elif kind == "strand":
            mates = [over[0][:3] + (over[0][3] ^ 1,) + over[0][4:]]
        elif kind == "break_good":               # an antisense mate hit whose flank would begin before the contig
            mates = [(1, 30, 130, 1 | 2, 0, 0, 100), over[0]]
        elif kind == "clip":                     # a sense mate hit ten bases before the contig's end
            mates = [(1, clen - 110, clen - 10, 2, 0, 0, 100)]
        elif kind == "two":
            mates = over[:2]
        elif kind == "m0":
            mates = []
        elif kind == "m3":
            mates = over[:3]
        elif kind == "nofirst":
            per_seg[0] = []
        if drop_first_mate:
            mates = mates[1:]
        for s in range(nseg):
            hits += per_seg[s]
            seg_off.append(len(hits))
        mate_hits += mates
        mate_off.append(len(mate_hits))
        assert len(seq) == rl
        reads.append(seq)
    seqg = "".join(g)
    n = len(kinds)
    seg_off = np.array(seg_off, dtype=np.uint32)
    mate_off = np.array(mate_off, dtype=np.uint32)
    lens = np.full(n, rl, dtype=np.int64)
    bases = np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy()
    if empty_between:
        at, count = empty_between
        seg_off = np.concatenate([seg_off[:(at + 1) * nseg + 1], np.full(count * nseg, seg_off[(at + 1) * nseg], dtype=np.uint32), seg_off[(at + 1) * nseg + 1:]])
        mate_off = np.concatenate([mate_off[:at + 2], np.full(count, mate_off[at + 1], dtype=np.uint32), mate_off[at + 2:]])
        bases = np.concatenate([bases[:(at + 1) * rl], np.zeros(count * L, dtype=np.uint8) + ord("A"), bases[(at + 1) * rl:]])
        lens = np.concatenate([lens[:at + 1], np.full(count, L, dtype=np.int64), lens[at + 1:]])
        n += count
    read_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    b = SegBatch(nseg, np.arange(1, n + 1, dtype=np.uint32), read_off, bases, seg_off, np.array(hits, dtype=HIT_DTYPE),
                 mate_off, np.array(mate_hits, dtype=HIT_DTYPE))
    return [seqg, g2], b


def params():
    return Params(read_side=READ_LEFT, inner_dist_mean=MEAN, inner_dist_std_dev=SD, max_segment_intron=400)


def oracle(kinds, nseg, **kw):
    seqs, b = make_batch(kinds, nseg, **kw)
    return orc.segjuncs(params(), orc.Genome(seqs), b)


@pytest.fixture(scope="module")
def planted():
    """the planted kinds on the CPU, the oracle alone: per kind and segment count (windows, rescue pairs) of eight reads of the kind"""
    n = 8
    sig = {}
    for nseg in (2, 3, 4):
        for kind in LISTED + NEIGHBOURS:
            st = oracle([kind] * n, nseg).stats
            sig[nseg, kind] = (st["windows"], st["rescue_pairs"])
        for kind in ("ok2", "ok3", "anti2", "anti3"):          # a pair that suits: scanned, a window a read
            assert sig[nseg, kind] == (n, n), (nseg, kind, sig[nseg, kind])
        assert sig[nseg, "two"] == (2 * n, 2 * n), (nseg, sig[nseg, "two"])
        for kind in ("contig", "strand", "m0", "nofirst"):      # no pair that suits, no mate hit, no hit to pair: nothing scanned
            assert sig[nseg, kind] == (0, 0), (nseg, kind, sig[nseg, kind])
        for kind in ("clip", "abut", "near", "far"):           # scanned, and no window: cut off, abutting, too near, too far
            assert sig[nseg, kind] == (0, n), (nseg, kind, sig[nseg, kind])
        # the break: nothing counted and the good second mate hit not reached -- which alone gives a window a read
        assert sig[nseg, "break_good"] == (0, 0), (nseg, sig[nseg, "break_good"])
        st = oracle(["break_good"] * n, nseg, drop_first_mate=True).stats
        assert (st["windows"], st["rescue_pairs"]) == (n, n), (nseg, st)
        assert sig[nseg, "m3"][1] == 3 * n and sig[nseg, "m3"][0] > 0, (nseg, sig[nseg, "m3"])
    return sig


@pytest.fixture(scope="module")
def lib():
    return host.load_lib()   # fails loudly when the extension is missing


def check(seqs, b, what):
    p = params()
    want = orc.segjuncs(p, orc.Genome(seqs), b)
    with host.Context(0) as ctx:
        ctx.upload_genome(host.pack_genome(seqs))
        got = ctx.segjuncs([(p, ctx.upload_batch(b))])
    print(what, {k: got.stats[k] for k in ("windows", "indel_pairs", "rescue_pairs", "overflow_blocks")}, len(want.juncs), len(want.deletions), len(want.insertions))
    assert_events_equal(got, want, what)
    for k in ("windows", "indel_pairs", "rescue_pairs"):
        assert got.stats[k] == want.stats[k], (what, k)
    return want


def tile(n_listed, k0=0):
    """256 reads, the first n_listed of them listed (every kind in turn), the others neighbours"""
    return [LISTED[(k0 + k) % len(LISTED)] for k in range(n_listed)] + [NEIGHBOURS[k % len(NEIGHBOURS)] for k in range(256 - n_listed)]


@pytest.mark.parametrize("nseg", [2, 3, 4])
def test_kinds_and_neighbours(lib, planted, nseg):
    """every kind and neighbour, interleaved, in a batch of three tiles (the last one short)"""
    kinds = [(LISTED + NEIGHBOURS)[k % 15] for k in range(600)]
    seqs, b = make_batch(kinds, nseg, seed=20 + nseg)
    want = check(seqs, b, "kinds, nseg %d" % nseg)
    assert want.stats["windows"] >= 200 and want.stats["rescue_pairs"] >= 400
    assert len(want.juncs) > 0


def test_slice_counts(lib, planted):
    """seven tiles whose workgroups list 0, 1, 63, 64, 65, 255 and 256 reads"""
    counts = (0, 1, 63, 64, 65, 255, 256)
    kinds = [k for i, c in enumerate(counts) for k in tile(c, 5 * i)]
    seqs, b = make_batch(kinds, 3, seed=31)
    assert b.n_reads == 256 * len(counts)
    want = check(seqs, b, "slice counts")
    assert want.stats["rescue_pairs"] >= sum(counts) // 2


def test_single_tile(lib, planted):
    seqs, b = make_batch(tile(65), 4, seed=32)
    want = check(seqs, b, "single tile")
    assert want.stats["windows"] > 0


def test_slice_of_257(lib, planted):
    """2 048 tiles: workgroup 0 of 2 047 takes the first and the last -- 256 listed reads and one more, its slice's second round"""
    kinds = tile(256) + ["ok3"]
    seqs, b = make_batch(kinds, 4, seed=33, empty_between=(255, 2047 * 256 - 256))
    assert b.n_reads == 2047 * 256 + 1
    want = check(seqs, b, "slice of 257")
    assert want.stats["windows"] >= 100
