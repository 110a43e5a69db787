"""A small --fusion-search case for long_spanning_reads, written from scratch: random contigs; chimeric reads of two 50-base pieces from
unrelated places (each piece on either strand, so the four fusion directions come up about equally often; the break lies on a
segment boundary, so every 25-base segment has a plain hit); plain and spliced reads in between; the segment maps and the reads as
BAM with `.index` side files (so the run can be cut into shards); the junction list of the spliced reads; and the `.fusions` list
stage 1 reports for these segment hits (the CPU oracle's find_fusions over the same records).  Test helper; make_case's
numbers scale it up for measuring the device writer against the host encoder."""
import gzip
import os
import struct
import zlib

import numpy as np

import orc
from tophat_amd.bamio import write_bam_from_sam
from tophat_amd.batch import build_seg_batch, build_span_batch
from tophat_amd.params import Params
from tophat_amd.samtext import md_nm, parse_sam_hits, sam_header

SEG = 25
RL = 100
FUSION_MIN_DIST = 300
_RC = str.maketrans("ACGT", "TGCA")


def revcomp(s):
    return s.translate(_RC)[::-1]


def rewrap_with_index(bam, every):
    """the BAM written by write_bam_from_sam cut again the way samtools cuts it -- the header in members of its own, no record across two
    members -- plus its `.index`: `read id \\t virtual offset` at a read-id change, `every` records or more after the last line"""
    data = gzip.open(bam, "rb").read()
    l_text, = struct.unpack_from("<i", data, 4)
    off = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, off)
    off += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", data, off)
        off += 8 + l_name
    members, index = [data[:off]], []
    cur, since, last_id = bytearray(), every, None
    while off < len(data):
        bs, = struct.unpack_from("<i", data, off)
        rec = data[off:off + 4 + bs]
        off += 4 + bs
        l_rn = rec[12]
        rid = int(rec[36:36 + l_rn - 1].split(b"|")[0])
        if len(cur) + len(rec) > 0xFF00 and cur:
            members.append(bytes(cur)); cur = bytearray()
        if since >= every and rid != last_id:
            index.append((rid, len(members), len(cur)))
            since = 0
        cur += rec
        since += 1
        last_id = rid
    if cur:
        members.append(bytes(cur))
    starts, at = [], 0
    with open(bam, "wb") as f:
        for m in members + [b""]:
            co = zlib.compressobj(1, zlib.DEFLATED, -15)
            comp = co.compress(m) + co.flush()
            blk = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(m) & 0xFFFFFFFF, len(m))
            starts.append(at)
            at += len(blk)
            f.write(blk)
    with open(bam + ".index", "w") as f:
        for rid, m, o in index:
            f.write("%d\t%d\n" % (rid, (starts[m] << 16) | o))


def make_case(d, n_chimeric=400, n_plain=400, seed=5, contig_len=6000, index_every=100, oracle=True):
    """-> dict: the files' paths (ref, hdr, reads, segs, juncs, insertions, deletions, fusions), names, and -- oracle=True -- `alns`:
    what the CPU oracle's long_spanning_reads gives for the case, with `read_ids`"""
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(seed)
    names = ["chrA", "chrB", "chrC"]
    seqs = ["".join(rng.choice(list("ACGT"), contig_len)) for _ in names]
    with open(os.path.join(d, "ref.fa"), "w") as f:
        for n, s in zip(names, seqs):
            f.write(">%s\n" % n)
            for k in range(0, len(s), 60):
                f.write(s[k:k + 60] + "\n")
    hdr = sam_header(names, [contig_len] * len(names))
    open(os.path.join(d, "hdr.sam"), "w").write(hdr)
    kinds = ["chimeric"] * n_chimeric + ["plain", "spliced"] * (n_plain // 2)
    rng.shuffle(kinds)
    seg_lines = [[] for _ in range(RL // SEG)]
    fq, juncs = [], set()

    def piece(n):
        """n bases of a random place on either strand -> (bases as the read has them, contig, left, reverse strand)"""
        c = int(rng.integers(0, len(names)))
        g = int(rng.integers(0, contig_len - n))
        rev = bool(rng.integers(0, 2))
        s = seqs[c][g:g + n]
        return (revcomp(s) if rev else s), c, g, rev

    for rid, kind in enumerate(kinds, 1):
        if kind == "chimeric":
            parts = [piece(RL // 2), piece(RL // 2)]
        elif kind == "plain":
            parts = [piece(RL)]
        else:                                                   # two exons of one transcript, an intron of 60..400 bases between them
            c = int(rng.integers(0, len(names)))
            intron = int(rng.integers(60, 400))
            g = int(rng.integers(0, contig_len - RL - intron))
            rev = bool(rng.integers(0, 2))
            a, b = (seqs[c][g:g + 50], c, g, rev), (seqs[c][g + 50 + intron:g + 100 + intron], c, g + 50 + intron, rev)
            parts = [(revcomp(b[0]),) + b[1:], (revcomp(a[0]),) + a[1:]] if rev else [a, b]
            juncs.add((names[c], g + 49, g + 50 + intron, "-" if rng.integers(0, 2) else "+"))
        read = list("".join(p[0] for p in parts))
        mism_at = int(rng.integers(0, RL)) if kind == "chimeric" and rng.random() < 0.1 else -1
        if mism_at >= 0:
            read[mism_at] = "ACGT"[("ACGT".index(read[mism_at]) + 1) % 4]
        read = "".join(read)
        qual = "".join(chr(int(x)) for x in rng.integers(35, 74, RL))
        fq.append((rid, read, qual))
        at = 0
        for text, c, g, rev in parts:
            for k in range(0, len(text), SEG):
                s = (at + k) // SEG
                seg = read[at + k:at + k + SEG]
                left = g + len(text) - k - SEG if rev else g + k
                fwd = revcomp(seg) if rev else seg
                nm, md = md_nm(seqs[c][left:left + SEG], fwd)
                seg_lines[s].append("\t".join(["%d|%d:%d:%d" % (rid, s * SEG, s, RL // SEG), "16" if rev else "0", names[c], str(left + 1), "255", "%dM" % SEG, "*", "0", "0",
                                               fwd, (qual[at + k:at + k + SEG][::-1] if rev else qual[at + k:at + k + SEG]), "NM:i:%d" % nm, "MD:Z:%s" % md]))
            at += len(text)
    out = {"dir": d, "names": names, "seqs": seqs, "ref": os.path.join(d, "ref.fa"), "hdr": os.path.join(d, "hdr.sam"), "segs": [], "n_reads": len(kinds),
           "chimeric_ids": [rid for rid, k in enumerate(kinds, 1) if k == "chimeric"]}
    seg_sams = []
    for s, lines in enumerate(seg_lines):
        sam = os.path.join(d, "seg%d.sam" % (s + 1))
        open(sam, "w").write(hdr + "\n".join(lines) + "\n")
        bam = os.path.join(d, "seg%d.bam" % (s + 1))
        write_bam_from_sam(sam, bam)
        rewrap_with_index(bam, index_every)
        out["segs"].append(bam)
        seg_sams.append(sam)
    rsam = os.path.join(d, "reads.sam")
    with open(rsam, "w") as f:
        f.write("@HD\tVN:1.0\tSO:unsorted\n")
        for rid, read, qual in fq:
            f.write("\t".join([str(rid), "4", "*", "0", "0", "*", "*", "0", "0", read, qual]) + "\n")
    out["reads"] = os.path.join(d, "reads.bam")
    write_bam_from_sam(rsam, out["reads"])
    rewrap_with_index(out["reads"], index_every)
    out["juncs"] = os.path.join(d, "case.juncs")
    open(out["juncs"], "w").write("".join("%s\t%d\t%d\t%s\n" % j for j in sorted(juncs)))
    for k in ("insertions", "deletions"):
        out[k] = os.path.join(d, "case." + k)
        open(out[k], "w").close()
    # stage 1 on the CPU: the break points find_fusions reports for these segment hits
    ref_ids = {n: i + 1 for i, n in enumerate(names)}
    reads = {rid: read for rid, read, _ in fq}
    seg_recs = [list(parse_sam_hits(s, ref_ids)) for s in seg_sams]
    g = orc.Genome(seqs)
    p1 = Params(read_side=1, segment_length=SEG, fusion_min_dist=FUSION_MIN_DIST)
    fus = orc.fusions(p1, g, build_seg_batch(seg_recs, reads, include_top0=True), p1.fusion_anchor_length, p1.fusion_min_dist)
    out["fusions"] = os.path.join(d, "case.fusions")
    orc.write_fusions(fus, names, out["fusions"])
    if oracle:
        from tophat_amd.host import JUNC_DTYPE
        sb = build_span_batch(seg_recs, reads, {rid: qual for rid, _, qual in fq})
        jr = np.array(sorted((ref_ids[n], l, r, 1 if s == "-" else 0) for n, l, r, s in juncs), dtype=JUNC_DTYPE)
        p2 = Params(fusion_search=1, fusion_min_dist=FUSION_MIN_DIST, segment_length=SEG)
        out["alns"] = orc.spanning_fusion(p2, g, sb, jr, [], orc.read_fusions_file(out["fusions"], ref_ids), True)
        out["read_ids"] = sb.read_id
    return out


def lsr_command(bindir, case, out_bam):
    return [os.path.join(bindir, "long_spanning_reads"), "--segment-length", str(SEG), "--sam-header", case["hdr"], "--fusion-search", "--fusion-min-dist", str(FUSION_MIN_DIST),
            case["ref"], case["reads"], case["juncs"], case["insertions"], case["deletions"], case["fusions"], out_bam, ",".join(case["segs"])]


def direction_of(cigar_text):
    """ff / fr / rf / rr of a fusion alignment from XF:Z's cigar text: lower-case ops run down the contig"""
    a, b = cigar_text.split("F", 1)
    a = a.rstrip("0123456789")
    return ("r" if any(ch.islower() for ch in a) else "f") + ("r" if any(ch.islower() for ch in b) else "f")
