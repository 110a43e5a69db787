"""CPU: the device BAM writer's fusion records (tophat_amd/csrc/thj_bamenc_fusion.h, compiled for the CPU by tests/xfsim: a wave of
64 fibers per fusion alignment under tests/hostsim/simt.h, into a buffer of stale bytes) against the executables' host encoder
(encode_aln, host/thj_bamrec.h: print_bamhit + extract_partial_hits) on a planted batch: the same byte stream, record sizes and
read ids, the bytes behind the stream untouched, every record readable by tophat_amd.bamio and -- restated here from the format --
carrying the piece of the read, the CIGAR and the XF:Z text its direction asks for.  The same program runs once more under the
address and undefined-behaviour sanitizers, as a process of its own."""
import os
import struct
import subprocess

import numpy as np
import pytest

from locked_make import locked_make
from tophat_amd.bamio import parse_bam_record
from tophat_amd.host import ALN_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
FF, FR, RF, RR = 7, 8, 9, 10
MD_ON_HOST = 255
HOST_ENCODER = 3                       # xfsim's exit code for "a record needs the host encoder"
NT16 = "=ACMGRSVTWYHKDBN"
LETTER = {1: "M", 2: "m", 3: "I", 4: "i", 5: "D", 6: "d", 7: "F", 8: "F", 9: "F", 10: "F", 11: "N", 12: "n", 13: "S"}
BAM_LETTER = {1: "M", 2: "M", 3: "I", 4: "I", 5: "D", 6: "D", 11: "N", 12: "N", 13: "S"}
CONTIGS = ["c", "chr_" + "abcdefghijklmnopqrstuvwxyz0123456789", "chr2", "chrX"]       # names of 1 and of 40 characters
assert len(CONTIGS[1]) == 40


@pytest.fixture(scope="module")
def exes():
    d = os.path.join(HERE, "xfsim")
    locked_make(d)
    return os.path.join(d, "xfsim"), os.path.join(d, "xfsim_san")


def revcomp(s):
    return "".join({"A": "T", "C": "G", "G": "C", "T": "A"}.get(ch, "N") for ch in reversed(s))


def read_record(name, seq, qual):
    """an unaligned read as the reads BAM holds it (flag 4, no cigar), block_size word included"""
    nib = [NT16.index(ch) for ch in seq] + [0]
    packed = bytes((nib[2 * k] << 4) | nib[2 * k + 1] for k in range((len(seq) + 1) // 2))
    nm = name.encode() + b"\0" if name is not False else b""          # False: a record without a name field (l_read_name 0)
    body = struct.pack("<iiIIiiii", -1, -1, (4680 << 16) | len(nm), 4 << 16, len(seq), -1, -1, 0) + nm + packed + qual + b"ZTZextra\0"
    return struct.pack("<I", len(body)) + body


class Batch:
    def __init__(self):
        self.rng = np.random.default_rng(20)
        self.reads, self.infl, self.loc, self.alns, self.labels = [], b"", [], [], []

    def read(self, n, name=None):
        """a read of n bases with an N and a non-ACGTN letter near both ends (so in either piece of any cut) -> its row"""
        seq = list(self.rng.choice(list("ACGT"), n))
        for at, ch in ((1, "N"), (3, "M"), (n - 2, "N"), (n - 4, "R"), (n // 2, "=")):
            seq[at] = ch
        qual = bytes(int(x) for x in self.rng.integers(2, 41, n))
        name = name if name is not None else str(1000 + 7 * len(self.reads))
        self.infl += b"\xEE" * int(self.rng.integers(0, 5))             # records do not start aligned
        self.loc.append(len(self.infl))
        self.infl += read_record(name, "".join(seq), qual)
        self.reads.append((name, "".join(seq), qual))
        return len(self.reads) - 1

    def aln(self, label, row, ref, left, ops, ref2=0, anti=False, xs_minus=False, AS=0, md=b"", mism=0, n_cigar=None, md_len=None):
        a = np.zeros(1, dtype=ALN_DTYPE)[0]
        a["read_idx"], a["ref_id"], a["left"] = row, ref, left
        a["flags"] = (1 if anti else 0) | (4 if xs_minus else 0)
        a["mismatches"], a["n_cigar"] = mism, len(ops) if n_cigar is None else n_cigar
        a["AS"], a["XM"], a["XO"], a["XG"] = AS, mism, 1 if any(3 <= op <= 6 for op, _ in ops) else 0, sum(l for op, l in ops if 3 <= op <= 6)
        a["md_len"] = len(md) if md_len is None else md_len
        a["md"] = md
        a["cigar"][:len(ops)] = [(op << 28) | l for op, l in ops]
        if ref2:
            a["cigar"][15] = ref2
        self.alns.append(a)
        self.labels.append(label)

    def file(self, path):
        names = b"".join(n.encode() + b"\0" for n in CONTIGS)
        alns = np.array(self.alns, dtype=ALN_DTYPE)
        with open(path, "wb") as f:
            f.write(struct.pack("<5I", len(CONTIGS), len(alns), len(self.loc), len(self.infl), len(names)))
            f.write(names + alns.tobytes() + np.asarray(self.loc, np.uint32).tobytes() + self.infl)
        return alns


def planted():
    b = Batch()
    lens = [50, 75, 100, 101, 150, 512]
    rows = {n: b.read(n) for n in lens}
    blank = b.read(100, name=" 4242")                                  # atol skips the leading blank
    k = 0
    # every direction, sense and antisense, one contig and two, odd and even cuts, every read length
    for d in (FF, FR, RF, RR):
        for anti in (False, True):
            n = lens[k % len(lens)]
            lp = n // 2 + (k & 1)
            ref, ref2 = 1 + k % 4, 1 + (k % 4 if k & 2 else (k + 1) % 4)
            b.aln("dir%d_anti%d" % (d, anti), rows[n], ref, 500 + 13 * k, [(1, lp), (d, 7000 + k), (1, n - lp)], ref2, anti, AS=-6 * k, md=b"%d" % n)
            b.aln("plain_after_%d" % k, rows[lens[(k + 1) % len(lens)]], 2, 100 + k, [(1, lens[(k + 1) % len(lens)])], md=b"%d" % lens[(k + 1) % len(lens)])
            k += 1
    # the remaining read lengths, in a direction that reverses both pieces, cut at an odd and at an even base
    for n in lens:
        for lp in (n // 2, n // 2 + 1):
            b.aln("len%d_cut%d" % (n, lp), rows[n], 3, 12345, [(2, lp), (RR, 3000), (2, n - lp)], 2, anti=bool(lp & 1), md=b"%d" % n)
    # fifteen ops: pieces with m i d n ops (reversed order, upper-casing), a soft clip, a spliced piece (XS)
    before = [(13, 4), (1, 10), (5, 2), (1, 8), (3, 1), (1, 9), (11, 120)]
    after = [(2, 10), (6, 3), (2, 5), (4, 2), (2, 8), (12, 99999), (2, 18)]
    for d in (FF, FR, RF, RR):
        b.aln("fifteen_ops_%d" % d, rows[75], 2, 99998, before + [(d, 99999)] + after, 4, anti=d in (FR, RF), xs_minus=d in (FF, FR), AS=-300,
              md=b"10^AC8A8^TTT10C12", mism=2)
    b.aln("plain_spliced", rows[100], 1, 77, [(1, 60), (11, 900), (1, 40)], md=b"100")
    # the fusion op as op 1 and as op n_cigar - 2, with several ops on the other side
    b.aln("fusion_is_op_1", rows[101], 1, 9, [(1, 9), (FR, 9), (2, 10), (12, 100000), (2, 41), (6, 1), (2, 41)], 2, md=b"101")
    b.aln("fusion_is_op_n_minus_2", rows[101], 4, 8, [(1, 51), (11, 99), (1, 40), (RF, 8), (1, 10)], 4, anti=True, md=b"101")
    b.aln("fusion_is_op_0", rows[50], 2, 50, [(FF, 5), (1, 50)], 3, md=b"50")
    # decimal widths: left 0 -> "1", second-contig position 0 -> "1F", 9 | 10, 99 | 100, 99999 | 100000
    for left, pos2, ln in ((0, 0, 9), (8, 8, 10), (9, 9, 99), (98, 98, 100), (99, 99, 50), (99998, 99998, 51), (99999, 99999, 75), (100000, 100000, 1)):
        b.aln("decimals_%d" % left, rows[150], 1, left, [(1, ln), (RF, pos2), (2, 150 - ln)], 1, md=b"150")
    # AS in every integer width, MD of 0, 24, 25 and 40 characters
    for AS, md in ((0, b""), (-127, b"1A" * 12), (-128, b"1A" * 12 + b"3"), (300, b"1A" * 20), (-32767, b"7"), (-32768, b"50")):
        b.aln("as%d_md%d" % (AS, len(md)), rows[50], 3, 4000, [(1, 20), (FR, 4100), (2, 30)], 1, anti=AS < -200, AS=AS, md=md, mism=len(md) // 2)
    b.aln("plain_antisense", blank, 4, 5, [(1, 100)], anti=True, md=b"100")
    b.aln("name_with_blank", blank, 4, 5, [(2, 33), (RR, 0), (1, 67)], 1, md=b"100")
    b.aln("plain_last", rows[512], 1, 0, [(1, 512)], md=b"512")
    return b


def run(exe, path, prefix):
    r = subprocess.run([exe, path, prefix], capture_output=True, text=True, timeout=300)
    dev = [(int(l.split()[1]), int(l.split()[2])) for l in r.stdout.split("\n") if l.startswith("D ")]
    hst = [(int(l.split()[1]), int(l.split()[2])) for l in r.stdout.split("\n") if l.startswith("H ")]
    return r, dev, hst


def expected_pieces(b, a):
    """(fi, [(contig, pos, cigar text, seq, qual)] x 2, XF:Z text after the record's number) of a fusion alignment"""
    name, seq, qual = b.reads[int(a["read_idx"])]
    ops = [(int(c) >> 28, int(c) & 0x0FFFFFFF) for c in a["cigar"][:int(a["n_cigar"])]]
    fi = next(i for i, (op, _) in enumerate(ops) if 7 <= op <= 10)
    d = ops[fi][0]
    if a["flags"] & 1:
        seq, qual = revcomp(seq), qual[::-1]
    lp = sum(l for op, l in ops[:fi] if 1 <= op <= 4)
    s1, q1, s2, q2 = seq[:lp], qual[:lp], seq[lp:], qual[lp:]
    c1, c2 = ops[:fi], ops[fi + 1:]
    if d in (RF, RR):
        s1, q1, c1 = revcomp(s1), q1[::-1], c1[::-1]
    if d in (FR, RR):
        s2, q2, c2 = revcomp(s2), q2[::-1], c2[::-1]
    right, fleft = int(a["left"]), None
    for op, l in ops:
        if op in (1, 11, 5):
            right += l
        elif op in (2, 12, 6):
            right -= l
        elif 7 <= op <= 10:
            fleft = right - 1 if op in (FF, FR) else right + 1
            right = l
    left1 = int(a["left"]) if d in (FF, FR) else fleft
    left2 = ops[fi][1] if d in (FF, RF) else right + 1
    n1, n2 = CONTIGS[int(a["ref_id"]) - 1], CONTIGS[int(a["cigar"][15]) - 1]
    text = "".join("%d%s" % (l + 1 if 7 <= op <= 10 else l, LETTER[op]) for op, l in ops)
    xf = " %s-%s %d %s %s %s" % (n1, n2, int(a["left"]) + 1, text, seq, "".join(chr(q + 33) for q in qual))
    cig = lambda c: "".join("%d%s" % (l, BAM_LETTER[op]) for op, l in c) or "*"
    return fi, [(n1, left1 + 1, cig(c1), s1, q1), (n2, left2 + 1, cig(c2), s2, q2)], xf


def test_planted_batch_matches_the_host_encoder(exes, tmp_path):
    b = planted()
    alns = b.file(str(tmp_path / "batch.bin"))
    r, dev, hst = run(exes[0], str(tmp_path / "batch.bin"), str(tmp_path / "out"))
    assert r.returncode == 0 and r.stdout.strip().endswith("SAME"), (r.returncode, r.stdout[-300:], r.stderr[-300:])
    dbytes = open(str(tmp_path / "out.dev"), "rb").read()
    hbytes = open(str(tmp_path / "out.host"), "rb").read()
    assert dbytes == hbytes
    assert dev == hst, "record sizes and read ids"
    fusion = [any(7 <= (int(c) >> 28) <= 10 for c in a["cigar"][:int(a["n_cigar"])]) for a in alns]
    assert len(dev) == len(alns) + sum(fusion) and sum(s for s, _ in dev) == len(dbytes)
    # the planted edges are in the batch
    seen_dirs = {(int(a["cigar"][1]) >> 28, int(a["flags"]) & 1, int(a["ref_id"]) == int(a["cigar"][15])) for a, l in zip(alns, b.labels) if l.startswith("dir")}
    assert {(d, s) for d, s, _ in seen_dirs} == {(d, s) for d in (FF, FR, RF, RR) for s in (0, 1)} and {c for _, _, c in seen_dirs} == {True, False}
    assert {int(a["md_len"]) for a in alns} >= {0, 24, 25, 40} and any(int(a["n_cigar"]) == 15 for a in alns)
    # every record is well-formed BAM and says what its direction asks for; the header lists the contigs in reverse order
    names = CONTIGS[::-1]
    at, k = 0, 0
    for a, is_f, label in zip(alns, fusion, b.labels):
        rname, rseq, rqual = b.reads[int(a["read_idx"])]
        if not is_f:
            rec = parse_bam_record(dbytes[at + 4:at + dev[k][0]], names)
            assert rec[0] == rname and rec[2] == CONTIGS[int(a["ref_id"]) - 1] and not any(t.startswith("XF:") for t in rec[8:]), label
            assert dev[k][1] == int(rname)
            at += dev[k][0]; k += 1
            continue
        fi, pieces, xf = expected_pieces(b, a)
        for part in (0, 1):
            size, rid = dev[k]
            assert struct.unpack_from("<I", dbytes, at)[0] == size - 4, label
            rec = parse_bam_record(dbytes[at + 4:at + size], names)
            contig, pos, cig, seq, qual = pieces[part]
            pos = max(pos, 0)                                  # (GBamRecord writes a position before the contig's start as -1)
            assert rid == int(rname) and rec[0] == rname, label
            assert rec[1] == (0x10 if a["flags"] & 1 else 0) and rec[4] == 255, label
            assert (rec[2], rec[3], rec[5]) == (contig, pos, cig), "%s, record %d: %r" % (label, part + 1, rec[:6])
            assert rec[6] == seq and rec[7] == "".join(chr(q + 33) for q in qual), "%s, record %d" % (label, part + 1)
            tags = list(rec[8:])
            assert [t[:2] for t in tags] == ["AS", "XM", "XO", "XG", "MD", "NM"] + (["XS"] if any(op in (11, 12) for op in (int(c) >> 28 for c in a["cigar"][:int(a["n_cigar"])])) else []) + ["XF"], label
            assert tags[0] == "AS:i:%d" % int(a["AS"]) and tags[4] == "MD:Z:" + bytes(a["md"])[:int(a["md_len"])].decode(), label
            assert tags[-1] == "XF:Z:%d%s" % (part + 1, xf), "%s, record %d: %s" % (label, part + 1, tags[-1])
            at += size; k += 1
    assert at == len(dbytes) and k == len(dev)
    by_label = dict(zip(b.labels, alns))
    assert expected_pieces(b, by_label["decimals_0"])[2].split(" ")[2:4] == ["1", "9M1F141m"]
    assert expected_pieces(b, by_label["fusion_is_op_0"])[1][0][2:4] == ("*", "")


def test_planted_batch_under_the_sanitizers(exes, tmp_path):
    """the sanitizer build as a process of its own: a read or write past any array's end, or undefined arithmetic, ends it with an error"""
    b = planted()
    b.file(str(tmp_path / "batch.bin"))
    r, dev, hst = run(exes[1], str(tmp_path / "batch.bin"), str(tmp_path / "san"))
    assert r.returncode == 0 and "SAME" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    assert dev == hst and len(dev) > len(b.alns)


@pytest.mark.parametrize("edit", ["md_on_host", "length_mismatch", "second_fusion_op", "ref_id2_zero", "ref_id2_past_the_end", "sixteen_ops", "empty_name"])
def test_what_stays_with_the_host_encoder(exes, tmp_path, edit):
    b = Batch()
    row = b.read(100)
    unnamed = b.read(100, name=False)
    b.aln("plain", row, 1, 10, [(1, 100)], md=b"100")
    ops = [(1, 40), (FR, 900), (2, 60)]
    if edit == "md_on_host":
        b.aln(edit, row, 1, 10, ops, 2, md_len=MD_ON_HOST)
    elif edit == "length_mismatch":
        b.aln(edit, row, 1, 10, [(1, 40), (FR, 900), (2, 59)], 2, md=b"99")
    elif edit == "second_fusion_op":
        b.aln(edit, row, 1, 10, [(1, 40), (FR, 900), (2, 30), (FF, 70), (1, 30)], 2, md=b"100")
    elif edit == "ref_id2_zero":
        b.aln(edit, row, 1, 10, ops, 0, md=b"100")
    elif edit == "ref_id2_past_the_end":
        b.aln(edit, row, 1, 10, ops, len(CONTIGS) + 1, md=b"100")
    elif edit == "sixteen_ops":
        b.aln(edit, row, 1, 10, [(1, 40), (FR, 900)] + [(2, 8), (6, 1)] * 6 + [(2, 12), (6, 1)], 2, md=b"100")
    else:
        b.aln(edit, unnamed, 1, 10, ops, 2, md=b"100")
    b.aln("plain", row, 2, 10, [(1, 100)], md=b"100")
    b.file(str(tmp_path / "batch.bin"))
    r, dev, hst = run(exes[0], str(tmp_path / "batch.bin"), str(tmp_path / "out"))
    assert r.returncode == HOST_ENCODER and r.stdout.strip() == "HOST 1" and not dev and not hst, (r.returncode, r.stdout[-200:], r.stderr[-200:])
    assert not os.path.exists(str(tmp_path / "out.dev"))
