"""Test-only: hand-worked cases of the accepted-hits record rewrite (thj_junctions --accepted-hits-out).  Every expected record is
written out here field by field, by hand, from reading print_sam_for_single / rewrite_sam_record / add_auxData / GBamRecord -- not
through accepted_ref.py.  A case = settings, reads of (the generator's draw, hits in `hits` order as (ref_id, AlignStatus score,
input record)), and the records expected in output order, or the loud case.  Also the loud cases and a seeded crowd."""
import struct

import numpy as np

from ingest_cases import EQ, M, N, X, codes, cw, record, tag

NAMES = ["chrA", "chrB", "chrC"]                            # ref_id 1, 2, 3
HEADER = ["chrA", "chrB"]                                   # the output header: chrC has no @SQ line
SEQ = codes("ACGTACGTACGTACGTACGT")
SEQB = bytes([0x12, 0x48] * 5)                              # the same 20 bases, two a byte
Q30 = bytes([30]) * 20
M20 = [cw(M, 20)]
AUX = tag("NM", "C", 0) + tag("AS", "c", -5)                # what most inputs carry


def inp(name, tid, pos, flag=0, cigar=M20, aux=AUX, **kw):
    """an input record without its block_size field (bin 4680 and MAPQ 255: both are made anew)"""
    return record(name, tid=tid, pos=pos, flag=flag, cigar=cigar, seq=kw.pop("seq", SEQ), aux=aux, **kw)[4:]


def out(name, tid, pos, mapq, flag, aux, cigar=M20, bin_=4681, seq=SEQB, qual=Q30, l_seq=20):
    """an expected record, block_size first: every field as given"""
    name = name.encode() + b"\0"
    body = name + b"".join(struct.pack("<I", w) for w in cigar) + seq + qual + aux
    core = struct.pack("<iiBBHHHiiii", tid, pos, len(name), mapq, bin_, len(cigar), flag, l_seq, -1, -1, 0)
    return struct.pack("<i", len(core) + len(body)) + core + body


def case(label, reads, want, library_type=1, rg=""):
    return {"label": label, "cfg": {"library_type": library_type, "rg": rg, "names": NAMES, "header": HEADER}, "reads": reads, "want": want}


NH = lambda n: tag("NH", "C", n)                            # noqa: E731
HI = lambda k: tag("HI", "C", k)                            # noqa: E731


def cases():
    cs = []
    # one alignment: MAPQ 50, primary (no 0x100), no HI, no CC
    cs.append(case("one", [(7, [(1, -5, inp("r1", 0, 100))])], [out("r1", 0, 100, 50, 0, AUX + NH(1))]))
    # two alignments on two contigs, hits order B then A: index_vector puts chrA first; draw 4 % 2 = 0: hits[0] (chrB) is the primary
    cs.append(case("two_contigs", [(4, [(2, -5, inp("r2", 1, 500)), (1, -5, inp("r2", 0, 300))])],
                   [out("r2", 0, 300, 3, 0x100, AUX + NH(2) + tag("CC", "Z", "chrB") + tag("CP", "S", 501) + HI(0)),
                    out("r2", 1, 500, 3, 0, AUX + NH(2) + HI(1))]))
    # two on one contig: CC:Z:=; draw 3 % 2 = 1: hits[1]
    cs.append(case("same_contig", [(3, [(1, -5, inp("r3", 0, 100)), (1, -5, inp("r3", 0, 4000))])],
                   [out("r3", 0, 100, 3, 0x100, AUX + NH(2) + tag("CC", "Z", "=") + tag("CP", "S", 4001) + HI(0)),
                    out("r3", 0, 4000, 3, 0, AUX + NH(2) + HI(1))]))
    # n = 3, 4, 5: MAPQ 1, 1, 0; CP below 256 is a C
    for n, mq in ((3, 1), (4, 1), (5, 0)):
        hits = [(1, -5, inp("m%d" % n, 0, 10 * (k + 1))) for k in range(n)]
        want = []
        for k in range(n):
            nxt = tag("CC", "Z", "=") + tag("CP", "C", 10 * (k + 2) + 1) if k + 1 < n else b""
            want.append(out("m%d" % n, 0, 10 * (k + 1), mq, 0 if k == 2 else 0x100, AUX + NH(n) + nxt + HI(k)))
        cs.append(case("n%d" % n, [(2, hits)], want))
    # QNAME: /1 is cut, /abc is not (4 characters remain from the slash on); a/b/2 is cut at its LAST slash
    cs.append(case("qname", [(0, [(1, -5, inp("read/1", 0, 100))]), (0, [(1, -5, inp("r/abc", 0, 100))]), (0, [(1, -5, inp("a/b/2", 0, 100))])],
                   [out("read", 0, 100, 50, 0, AUX + NH(1)), out("r/abc", 0, 100, 50, 0, AUX + NH(1)), out("a/b", 0, 100, 50, 0, AUX + NH(1))]))
    # AS changes width both ways: c -> s (score -200), and a positive score -> 0, which is a C
    cs.append(case("AS_width", [(0, [(1, -200, inp("w1", 0, 100))]), (0, [(1, 3, inp("w2", 0, 100))])],
                   [out("w1", 0, 100, 50, 0, tag("NM", "C", 0) + tag("AS", "s", -200) + NH(1)), out("w2", 0, 100, 50, 0, tag("NM", "C", 0) + tag("AS", "C", 0) + NH(1))]))
    # NM stored as i comes out C; -127 c, -128 s, -32767 s, -32768 i; 255 C, 256 S, 65535 S, 65536 I; A and Z as they are
    wide = (tag("NM", "i", 1) + tag("ZA", "i", -127) + tag("ZB", "i", -128) + tag("ZC", "i", -32767) + tag("ZD", "i", -32768) + tag("ZE", "I", 255) + tag("ZF", "i", 256) +
            tag("ZG", "I", 65535) + tag("ZH", "S", 65535) + tag("ZI", "i", 65536) + tag("ZJ", "A", "q") + tag("ZK", "Z", "some text") + tag("AS", "i", -5))
    narrow = (tag("NM", "C", 1) + tag("ZA", "c", -127) + tag("ZB", "s", -128) + tag("ZC", "s", -32767) + tag("ZD", "i", -32768) + tag("ZE", "C", 255) + tag("ZF", "S", 256) +
              tag("ZG", "S", 65535) + tag("ZH", "S", 65535) + tag("ZI", "I", 65536) + tag("ZJ", "A", "q") + tag("ZK", "Z", "some text") + tag("AS", "c", -5))
    cs.append(case("int_widths", [(0, [(1, -5, inp("iw", 0, 100, aux=wide))])], [out("iw", 0, 100, 50, 0, narrow + NH(1))]))
    # an input NH and an XS:i are dropped; a Z value holding NH:i: is dropped
    cs.append(case("dropped", [(0, [(1, -5, inp("dr", 0, 100, aux=tag("NH", "C", 9) + AUX + tag("XS", "c", -3) + tag("ZZ", "Z", "was NH:i:4 once") + tag("YT", "Z", "UU")))])],
                   [out("dr", 0, 100, 50, 0, AUX + tag("YT", "Z", "UU") + NH(1))]))
    # the strand tag: fr-firststrand antisense +, sense -; fr-secondstrand antisense -, sense +; none under fr-unstranded; an XS:A of the
    # input stays and keeps it away, and so does a Z value that holds XS:A:
    for lib, anti, ch in ((2, True, "+"), (2, False, "-"), (3, True, "-"), (3, False, "+")):
        cs.append(case("strand_%d_%d" % (lib, anti), [(0, [(1, -5, inp("st", 0, 100, flag=0x10 if anti else 0))])],
                       [out("st", 0, 100, 50, 0x10 if anti else 0, AUX + NH(1) + tag("XS", "A", ch))], library_type=lib))
    cs.append(case("strand_unstranded", [(0, [(1, -5, inp("st", 0, 100, flag=0x10))])], [out("st", 0, 100, 50, 0x10, AUX + NH(1))]))
    cs.append(case("strand_given", [(0, [(1, -5, inp("st", 0, 100, aux=AUX + tag("XS", "A", "+")))])], [out("st", 0, 100, 50, 0, AUX + tag("XS", "A", "+") + NH(1))], library_type=2))
    cs.append(case("strand_in_Z", [(0, [(1, -5, inp("st", 0, 100, aux=AUX + tag("CO", "Z", "see XS:A:-")))])], [out("st", 0, 100, 50, 0, AUX + tag("CO", "Z", "see XS:A:-") + NH(1))],
                   library_type=3))
    # --rg-id comes last, behind HI
    cs.append(case("rg", [(1, [(1, -5, inp("g", 0, 100)), (1, -5, inp("g", 0, 200))])],
                   [out("g", 0, 100, 3, 0x100, AUX + NH(2) + tag("CC", "Z", "=") + tag("CP", "C", 201) + tag("XS", "A", "-") + HI(0) + tag("RG", "Z", "grp1")),
                    out("g", 0, 200, 3, 0, AUX + NH(2) + tag("XS", "A", "-") + HI(1) + tag("RG", "Z", "grp1"))], library_type=2, rg="grp1"))
    # = and X become M (the ops are not merged); the bin is made anew: pos 16380 + 8 + 2 + 5000 + 10 crosses a 16 kb bin -> 585
    cs.append(case("cigar_bin", [(0, [(1, -5, inp("cb", 0, 16380, cigar=[cw(EQ, 8), cw(X, 2), cw(N, 5000), cw(M, 10)]))])],
                   [out("cb", 0, 16380, 50, 0, AUX + NH(1), cigar=[cw(M, 8), cw(M, 2), cw(N, 5000), cw(M, 10)], bin_=585)]))
    # QUAL beginning 0xff: 0xff throughout; an odd length's spare nibble comes out 0
    cs.append(case("qual_ff", [(0, [(1, -5, inp("qf", 0, 100, qual=bytes([0xFF, 7]) + bytes(18)))])], [out("qf", 0, 100, 50, 0, AUX + NH(1), qual=bytes([0xFF]) * 20)]))
    cs.append(case("odd_length", [(0, [(1, -5, inp("od", 0, 100, cigar=[cw(M, 3)], seq=codes("ACG"), spare=9))])],
                   [out("od", 0, 100, 50, 0, AUX + NH(1), cigar=[cw(M, 3)], seq=bytes([0x12, 0x40]), qual=bytes([30]) * 3, l_seq=3)]))
    # a tie on (contig, left) with n <= 16: the two stand in hits order (the second has the longer cigar), behind the one on the left
    tie = [(1, -5, inp("t", 0, 700)), (1, -5, inp("t", 0, 700, cigar=[cw(M, 10), cw(M, 10)])), (1, -5, inp("t", 0, 300))]
    cs.append(case("tie", [(5, tie)],
                   [out("t", 0, 300, 1, 0, AUX + NH(3) + tag("CC", "Z", "=") + tag("CP", "S", 701) + HI(0)),
                    out("t", 0, 700, 1, 0x100, AUX + NH(3) + tag("CC", "Z", "=") + tag("CP", "S", 701) + HI(1)),
                    out("t", 0, 700, 1, 0x100, AUX + NH(3) + HI(2), cigar=[cw(M, 10), cw(M, 10)])]))
    return cs


def loud_cases():
    """(label, hits of one read, what the message names)"""
    big = inp("big", 0, 100, aux=AUX + tag("ZZ", "Z", "x" * 65440))
    return [
        ("fusion", [(1, -5, inp("f", 0, 100, aux=AUX + tag("XF", "Z", "1 chrA-chrB 101 10M90F10M ACGT IIII")))], "fusion"),
        ("type_f", [(1, -5, inp("f", 0, 100, aux=AUX + tag("ZF", "f", b"\0\0\0\0")))], "type f, d, H or B"),
        ("type_d", [(1, -5, inp("f", 0, 100, aux=AUX + tag("ZD", "d", bytes(8))))], "type f, d, H or B"),
        ("type_H", [(1, -5, inp("f", 0, 100, aux=AUX + tag("ZH", "H", "1AE3")))], "type f, d, H or B"),
        ("type_B", [(1, -5, inp("f", 0, 100, aux=AUX + tag("ZB", "B", ("c", [1, 2]))))], "type f, d, H or B"),
        ("empty_Z", [(1, -5, inp("f", 0, 100, aux=AUX + tag("ZE", "Z", "")))], "Z tag"),
        ("tab_in_Z", [(1, -5, inp("f", 0, 100, aux=AUX + tag("ZT", "Z", "a\tb")))], "Z tag"),
        ("no_bases", [(1, -5, inp("f", 0, 100, cigar=[], seq=[]))], "l_seq == 0"),
        ("mate", [(1, -5, inp("f", 0, 100, mtid=1))], "paired records: not built"),
        ("flag_1", [(1, -5, inp("f", 0, 100, flag=1))], "paired records: not built"),
        ("over_64k", [(1, -5, big), (1, -5, inp("big", 0, 200))], "over 64 KiB"),
        ("contig", [(3, -5, inp("f", 2, 100))], "@SQ"),
    ]


def crowd(seed=5, n_reads=300):
    """seeded reads of 1 .. 24 hits in shuffled hits order, tags of every integer width, random settings -> cases without `want`"""
    rng = np.random.default_rng(seed)
    out_ = []
    for r in range(n_reads):
        n = int(rng.choice([1, 1, 2, 3, 5, 16, 17, 24]))
        hits = []
        for k in range(n):
            ref = int(rng.integers(1, 3))
            pos = int(rng.integers(0, 40)) * 1000 if n <= 16 else 1000 * k + ref      # (beyond 16 no ties here: their order is std::sort's own)
            ln = int(rng.integers(1, 40))
            aux = b""
            for t in range(int(rng.integers(0, 6))):
                kind = int(rng.integers(0, 5))
                key = "Z%s" % "abcdefgh"[t]
                if kind == 0:
                    v = int(rng.choice([-40000, -32768, -32767, -129, -128, -127, -1, 0, 255, 256, 65535, 65536, 3000000000]))
                    ty = [x for x in "cCsSiI" if {"c": -128 <= v <= 127, "C": 0 <= v <= 255, "s": -32768 <= v <= 32767, "S": 0 <= v <= 65535, "i": -2 ** 31 <= v < 2 ** 31,
                                                  "I": 0 <= v < 2 ** 32}[x]]
                    aux += tag(key, ty[int(rng.integers(0, len(ty)))], v)
                elif kind == 1:
                    aux += tag(["NH", "XS", "AS", "NM"][int(rng.integers(0, 4))], "sS"[int(rng.integers(0, 2))], int(rng.integers(0, 300)))
                elif kind == 2:
                    aux += tag(key, "Z", ["x", "NH:i:", "has XS:i:1", "XS:A:+", "plain text of some length " * int(rng.integers(1, 9))][int(rng.integers(0, 5))])
                elif kind == 3:
                    aux += tag(["XS", "ZQ"][int(rng.integers(0, 2))], "A", "+-"[int(rng.integers(0, 2))])
                else:
                    aux += tag("AS", "cCsi"[int(rng.integers(0, 4))], int(rng.integers(0, 100)))
            name = ["q%d" % r, "q%d/1" % r, "q%d/12" % r, "q%d/123" % r, "/2"][int(rng.integers(0, 5))]
            cig = [[cw(M, ln)], [cw(EQ, ln - 1), cw(X, 1)] if ln > 1 else [cw(X, 1)], [cw(M, ln), cw(N, int(rng.integers(50, 70000))), cw(2, 3)]][int(rng.integers(0, 3))]
            qual = bytes([0xFF] * ln) if rng.integers(0, 8) == 0 else bytes(int(x) for x in rng.integers(0, 42, ln))
            rec = record(name, tid=ref - 1, pos=pos, flag=int(rng.choice([0, 0x10, 0x100, 0x410])), cigar=cig, seq=[int(x) for x in rng.integers(0, 16, ln)], qual=qual,
                         aux=aux, spare=int(rng.integers(0, 16)))[4:]
            hits.append((ref, int(rng.integers(-70000, 5)), rec))
        out_.append(case("crowd%d" % r, [(int(rng.integers(0, 2 ** 32)), hits)], None, library_type=int(rng.integers(1, 4)), rg=["", "rg7"][int(rng.integers(0, 2))]))
    return out_
