"""Test infrastructure: a plain-Python restatement of what tophat_reports does with its READS files -- the worker loop that walks the two
hit streams and the two read streams (tophat_reports.cpp:2324-2611), getQRead with the process() callback (reads.cpp:632-676,
tophat_reports.cpp:2197-2219), write_singleton_alignments (:2229-2322), writeUnmapped with um_written (reads.h:235-258), the record
GBamRecord makes through seqData's text (common.cpp:974-998, :1025-1109, :1249-1337), SAlignStats (:312-356) and print_alnStats
(:2119-2195).  Deliberately the LOOP, not the closed form the device uses.  The per-read and per-insert choice comes from best_ref.py and
pair_ref.py.  Written from reading the reference, each step citing its lines; nothing here runs on a GPU or calls the product.

A reads file = a list of raw BAM records (without their block_size fields), prep_reads' unaligned BAM.  A single-end run: side = best_cases'
form (recs, reads, AS, mism, anti) plus numbers[read] = the read's number.  A paired run: L, R in pair_cases' form (reads = the insert's
number inside the case), numbers[insert] likewise."""
from __future__ import annotations

import struct

import best_ref as br
import indelbed_ref as ir
import jbknown_ref as jr
import pair_ref as pr

STATS = ("num_aligned_left", "num_unmapped_left", "num_aligned_left_multi", "num_aligned_left_xmulti",
         "num_aligned_right", "num_unmapped_right", "num_aligned_right_multi", "num_aligned_right_xmulti",
         "num_aligned_pairs", "num_aligned_pairs_multi", "num_aligned_pairs_disc",
         "num_aligned_unpaired", "num_unmapped_unpaired", "num_aligned_unpaired_multi", "num_aligned_unpaired_xmulti")      # SAlignStats, :314-332
NT16_REV = "=ACMGRSVTWYHKDBN"                                   # bam_nt16_rev_table
NT16 = {c: 15 for c in map(chr, range(256))}                    # bam_nt16_table, bam_import.c:24-41
NT16.update({"=": 0, "0": 1, "1": 2, "2": 4, "3": 8})
for _k, _c in enumerate(NT16_REV[1:], 1):
    NT16[_c] = _k
    NT16[_c.lower()] = _k
SEQ_COMP = (0, 8, 4, 12, 2, 10, 9, 14, 1, 6, 5, 13, 3, 11, 7, 15)      # seqData, common.cpp:1250
SEEN = None                                                     # a dict: outcome class -> how often it was met (the crowd's self-check)


def _saw(what):
    if SEEN is not None:
        SEEN[what] = SEEN.get(what, 0) + 1


# ---- a read of the stream: bam2Read, QReadDataValue::init
def aux_find(aux, name):
    """bam_aux_get: the first tag of that name -> (type, value bytes) or None"""
    p = 0
    while p + 3 <= len(aux):
        key, ty = aux[p:p + 2], chr(aux[p + 2])
        v = p + 3
        if ty in "AcC":
            ln = 1
        elif ty in "sS":
            ln = 2
        elif ty in "iIf":
            ln = 4
        elif ty == "d":
            ln = 8
        elif ty in "ZH":
            ln = aux.index(b"\0", v) - v + 1
        elif ty == "B":
            ln = 5 + {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}[chr(aux[v])] * struct.unpack_from("<i", aux, v + 1)[0]
        else:
            raise ValueError("tag type %r" % ty)
        if key == name:
            return ty, aux[v:v + ln]
        p = v + ln
    return None


class QRead:
    """QReadDataValue (reads.h:149-176) with the Read bam2Read fills in (reads.cpp:518-525)"""

    def __init__(self, raw):
        tid, pos, l_qname, mapq, bin_, n_cigar, flag, l_seq, mtid, mpos, tlen = struct.unpack_from("<iiBBHHHiiii", raw, 0)
        p = 32
        qname = raw[p:p + l_qname - 1]; p += l_qname + 4 * n_cigar
        seq = raw[p:p + (l_seq + 1) // 2]; p += (l_seq + 1) // 2
        qual = raw[p:p + l_seq]; p += l_seq
        aux = raw[p:]
        self.id = int(qname.decode())                           # atol(rf.name), reads.cpp:533 (the tests' names are digits)
        self.matenum = 1 if flag & 0x40 else 2 if flag & 0x80 else 0      # reads.h:169-172: 0x1 is not looked at
        zt = aux_find(aux, b"ZT")
        self.trash = chr(zt[1][0]) if zt and zt[0] == "A" and zt[1][0] else None      # tag_char -> bam_aux2A
        zn = aux_find(aux, b"ZN")
        self.alt_name = zn[1][:-1].decode("latin-1") if zn else ""      # tag_str("ZN")
        self.um_written = False
        # seqData, common.cpp:1249-1337 (no colour space)
        codes = [(seq[i >> 1] >> (0 if i & 1 else 4)) & 15 for i in range(l_seq)]
        rev = bool(flag & 0x10)
        if rev:
            codes = [SEQ_COMP[c] for c in reversed(codes)]
        self.seq = "".join(NT16_REV[c] for c in codes)
        q = [ord("I") if b == 0xFF else (b + 33) & 0xFF for b in qual]
        if rev:
            q.reverse()
        self.qual = bytes(q)


def write_unmapped_record(rd):
    """GetReadProc::writeUnmapped's record (reads.h:237-256) with its block_size field: GBamRecord(rname, -1, 0, false, seq, NULL, qual)"""
    rname = rd.alt_name
    slash = rname.rfind("/")
    if slash != -1 and len(rname) - slash < 4:
        rname = rname[:slash]
    flag = 0x4                                                  # common.cpp:978-982: pos <= 0 -> unmapped, tid -1
    l_seq = len(rd.seq)                                         # strlen(qseq)
    sb = bytearray((l_seq + 1) // 2)                            # add_sequence, :1094-1096
    for i, ch in enumerate(rd.seq):
        sb[i >> 1] |= NT16[ch] << (4 * (1 - i % 2))
    if rd.qual == b"*":                                         # add_quals, :1104-1107
        qb = bytes([0xFF]) * l_seq
    else:
        qb = bytes((x - 33) & 0xFF for x in rd.qual[:l_seq])
    if rd.matenum:                                              # reads.h:243-247
        flag |= 0x1 | (0x40 if rd.matenum == 1 else 0x80)
    aux = b"ZTA" + rd.trash.encode() if rd.trash else b""       # :249-255
    name = rname.encode("latin-1") + b"\0"
    bin_ = (4681 + ((-1 & 0xFFFFFFFF) >> 14)) & 0xFFFF           # set_cigar without a CIGAR, :1078: bam_reg2bin(-1, 0) into a 16-bit field
    core = struct.pack("<iiBBHHHiiii", -1, -1, len(name), 0, bin_, 0, flag, l_seq, -1, -1, 0)
    body = name + bytes(sb) + qb + aux
    return struct.pack("<i", len(core) + len(body)) + core + body


class Proc:
    """CReadProc (:2197-2219) over GetReadProc (reads.h:215-261)"""

    def __init__(self, out, stats, um, mm, u_um, u_mm):
        self.out, self.stats, self.um, self.mm, self.u_um, self.u_mm = out, stats, um, mm, u_um, u_mm

    def write_unmapped(self, rd):
        if rd.um_written:
            return
        self.out.append(write_unmapped_record(rd))
        rd.um_written = True

    def process(self, rd, found):
        if rd.trash != "M" and not found:
            self.write_unmapped(rd)
        if not found:
            if rd.trash != "M":
                self.stats[self.um if rd.matenum else self.u_um] += 1
                _saw("no_group_unmapped")
            else:
                self.stats[self.mm if rd.matenum else self.u_mm] += 1
                _saw("no_group_ZT_M")


class ReadStream:
    """ReadStream::getQRead (reads.cpp:632-676) over an id-sorted file (the priority queue changes nothing then)"""

    def __init__(self, raws):
        self.q, self.at, self.last_id = [QRead(r) for r in raws], 0, 0

    def get(self, r_id, proc):
        assert r_id >= self.last_id, "getQRead() called with out-of-order id#"
        self.last_id = r_id
        found = None
        while found is None and self.at < len(self.q):
            rd = self.q[self.at]
            self.at += 1
            if rd.id == r_id:
                found = rd
            elif rd.id > r_id:
                self.at -= 1                                    # read_pq.push(rdata)
                break
            proc.process(rd, found is not None)
        return found


VMAX = 1 << 62


def read_best(S, idx, ctx, rng):
    """exclude_hits_on_filtered_junctions + read_best_alignments with final_report (:2286-2291, :113-212) over one read's records ->
    (map_flags, best_hits): best_ref.choose's second pass, one read"""
    max_multihits, suppress, mp = ctx["best"]
    cand = [k for k in idx if ctx["live"][S["tag"]][k] and ir.kept(S["recs"][k], ctx["accepted"])]
    sc = {k: br.score(S["recs"][k], S["AS"][k], ctx["js1"], ctx["known"], mp) for k in cand}
    top = max(sc.values(), default=None)
    ties = [k for k in cand if sc[k] == top]
    _srt, left = br.sort_unique(ties, S["recs"], S["mism"], S["anti"])
    code = 0
    if len(left) > max_multihits:
        code |= 16
        if suppress:
            left = []
        else:
            tie = list(range(len(left)))
            while len(tie) > max_multihits:
                del tie[rng() % len(tie)]
            left = [left[t] for t in tie]
    if left:
        code |= 1
        if len(left) > 1:
            code |= 4
    return code, left


def rescued_dist(h1, h2, junctions, keys, lo, hi):
    """inserts.h:111-150: the distance the first rescuing junction leaves, or None"""
    if h1.left < h2.left:
        inner1, inner2 = h1.right, h2.left
    else:
        inner1, inner2 = h2.right, h1.left
    import bisect
    lb = bisect.bisect_right(keys, (h1.ref, inner1 & ir.U32, inner1 & ir.U32, 1))
    ub = bisect.bisect_left(keys, (h1.ref, inner2 & ir.U32, inner2 & ir.U32, 0))
    while lb != ub and lb != len(keys):
        j = keys[lb]
        if inner1 <= ir._i32(j[1]) and inner2 >= ir._i32(j[2]) and junctions[j][2] >= 10:
            d = ir._i32(j[1]) - inner1 + inner2 - ir._i32(j[2])
            if lo <= d <= hi:
                return d
        lb += 1
    return None


def concordant(cands, ctx):
    """InsertAlignmentGrade::concordant() (inserts.h:222-225) of pair_best_alignments' best_grade: the first candidate in generation order
    that raised it (:443-447); a default grade (no candidate allowed) has num_mapped 0"""
    best = None
    for lh, rh, g in cands:
        if g is not None and (best is None or best[0] < g[0]):
            best = (g[0], g[1], lh, rh)
    if best is None:
        return False
    _sc, fusion, lh, rh = best
    mean, sd = ctx["pair"][0], ctx["pair"][1]
    inner = pr.inner_dist(lh, rh)
    if inner > mean + sd and not fusion:
        d = rescued_dist(lh, rh, ctx["js1"], ctx["keys1"], mean - sd, mean + sd)
        if d is not None:
            inner = d
    return lh.anti != rh.anti and inner <= ctx["max_report_intron"]


def make_ctx(L, R, best, pair=None, min_anchor=8, known=(), limits=None, max_report_intron=500000):
    """the first pass (best_ref / pair_ref) and what the second pass reads of it -> (L, R with their tags, ctx)"""
    PE = R is not None
    known = set(known)
    L = dict(L, tag="L")
    sides = {"L": L}
    if PE:
        R = dict(R, tag="R")
        sides["R"] = R
        ch = pr.choose(L, R, best, pair, min_anchor, known, limits)
    else:
        ch = br.choose(L["recs"], L["reads"], L["AS"], L["mism"], L["anti"], best, min_anchor, known, limits)
    ctx = dict(best=best, pair=pair, js1=ch["js1"], keys1=sorted(ch["js1"]), accepted=ch["accepted"], known=known, max_report_intron=max_report_intron, ch=ch,
               live={s: [not jr.dropped(S["mism"][i], S["recs"][i][3], limits) for i in range(len(S["recs"]))] for s, S in sides.items()})
    return L, R, ctx


def walk(L, R, left_reads, right_reads, numbers, best, pair=None, min_anchor=8, known=(), limits=None, max_report_intron=500000):
    """the worker's operator() (:2324-2611) -> (left unmapped records, right unmapped records, the fifteen counters).  R / right_reads /
    pair None: single-end input"""
    PE = R is not None
    L, R, ctx = make_ctx(L, R, best, pair, min_anchor, known, limits, max_report_intron)
    known, ch = ctx["known"], ctx["ch"]
    max_multihits, suppress, mp = best
    mixed, discordant = (pair[3], pair[4]) if PE else (False, False)
    stats = dict.fromkeys(STATS, 0)
    rng = br.Mt19937(1)                                         # :2325
    left_out, right_out = [], []
    left_file, right_file = ReadStream(left_reads), ReadStream(right_reads if PE else [])
    # the hit streams: a read's / an insert's records under its number, in rising number
    def stream(S):
        return [(numbers[S["reads"][s]], list(range(s, e))) for s, e in br.groups(S["reads"])] + [(VMAX, [])]
    lh, rh = stream(L), (stream(R) if PE else [(VMAX, [])])
    li = ri = 0
    l_proc = Proc(left_out, stats, "num_unmapped_left", "num_aligned_left_xmulti", "num_unmapped_unpaired" if PE else "num_unmapped_left",
                  "num_aligned_unpaired_xmulti" if PE else "num_aligned_left_xmulti")                      # :2378-2386
    r_proc = Proc(right_out, stats, "num_unmapped_right", "num_aligned_right_xmulti", "num_unmapped_unpaired", "num_aligned_unpaired_xmulti")
    lists = {}

    def singleton(obs, S, idx, file, frag, proc, got=None):
        """write_singleton_alignments, :2229-2322"""
        set_ = "left"
        if got is None:
            got = file.get(obs, proc)
        assert got is not None, "singleton getQRead() failed for id# %d" % obs
        if got.matenum == 0:
            if PE:
                set_ = "unpaired"
                _saw("matenum0_in_a_paired_run")
        elif frag == "R":
            set_ = "right"
        if PE and not mixed:                                    # :2266-2280
            proc.write_unmapped(got)
            stats["num_unmapped_" + set_] += 1
            _saw("alone_without_mixed")
            return
        code, hits = read_best(S, idx, ctx, rng)
        if code & 4:
            stats["num_aligned_%s_multi" % set_] += 1
        if code & 16:
            stats["num_aligned_%s_xmulti" % set_] += 1
        if code & 1:
            stats["num_aligned_" + set_] += 1
        else:
            if not got.um_written:
                stats["num_unmapped_" + set_] += 1
            proc.write_unmapped(got)
        _saw("read_over_the_cap_suppressed" if code == 16 else "read_over_the_cap" if code & 16 else "read_multi" if code & 4 else "read_aligned" if code & 1 else "read_nothing_left")
        if hits:
            if not got.um_written:
                rng()                                           # print_sam_for_single, :1005-1007
        else:
            proc.write_unmapped(got)

    while lh[li][0] != VMAX or rh[ri][0] != VMAX:
        while lh[li][0] < rh[ri][0] and lh[li][0] != VMAX:     # left singletons, :2396-2406
            singleton(lh[li][0], L, lh[li][1], left_file, "L" if PE else "U", l_proc)
            li += 1
        while lh[li][0] > rh[ri][0] and rh[ri][0] != VMAX:     # right singletons, :2409-2418
            singleton(rh[ri][0], R, rh[ri][1], right_file, "R", r_proc)
            ri += 1
        while lh[li][0] == rh[ri][0] and lh[li][0] != VMAX:    # both mates have alignments, :2422-2594
            obs, lidx, ridx = lh[li][0], lh[li][1], rh[ri][1]
            lhits = [k for k in lidx if ir.kept(L["recs"][k], ctx["accepted"])]            # exclude_hits_on_filtered_junctions, :2426-2430
            rhits = [k for k in ridx if ir.kept(R["recs"][k], ctx["accepted"])]
            paired = bool(lhits) and bool(rhits)                # :2434-2435
            l_read, r_read = left_file.get(obs, l_proc), right_file.get(obs, r_proc)
            assert l_read is not None and r_read is not None, "failed to retrieve a read for pair # %d" % obs
            flags, hits = 0, []
            if paired:
                lid, rid = [k for k in lhits if ctx["live"]["L"][k]], [k for k in rhits if ctx["live"]["R"][k]]      # the limits, inside pair_best_alignments
                lsc = {k: br.score(L["recs"][k], L["AS"][k], ctx["js1"], known, mp) for k in lid}
                rsc = {k: br.score(R["recs"][k], R["AS"][k], ctx["js1"], known, mp) for k in rid}
                pr.TRACE = []
                hits, best_fusion, over = pr.pair_best(L, R, lid, rid, lsc, rsc, ctx["js1"], ctx["keys1"], pair, best, True, rng)
                trace, pr.TRACE = pr.TRACE[-1], None
                nhits = len(hits) if not over else max_multihits + 1      # the list's length before the cap: only > 0, > 1, > max_multihits are read
                flags = (3 if nhits > 0 else 0) | (12 if nhits > 1 else 0) | (48 if nhits > max_multihits else 0)      # :526-536
                if (flags & 3) == 3 and not concordant(trace["cands"], ctx):      # :2485-2487
                    stats["num_aligned_pairs_disc"] += 1
                    _saw("discordant_pair")
                if mixed and (not hits or (best_fusion and not discordant)):      # :2488-2493
                    paired = False
                    _saw("mixed_gives_up_the_pairs")
            if paired:                                          # :2495-2564
                if hits:
                    lists[obs] = hits
                    rng()                                       # print_sam_for_pair, :1055-1056
                    l_read.um_written = r_read.um_written = True
                    stats["num_aligned_left"] += 1; stats["num_aligned_right"] += 1; stats["num_aligned_pairs"] += 1
                else:
                    stats["num_unmapped_left"] += 1; stats["num_unmapped_right"] += 1
                if flags & 4:
                    stats["num_aligned_left_multi"] += 1
                if flags & 8:
                    stats["num_aligned_right_multi"] += 1
                if (flags & 12) == 12:
                    stats["num_aligned_pairs_multi"] += 1
                if flags & 16:
                    stats["num_aligned_left_xmulti"] += 1
                if flags & 32:
                    stats["num_aligned_right_xmulti"] += 1
                if not flags & 1:
                    l_proc.write_unmapped(l_read)
                if not flags & 2:
                    r_proc.write_unmapped(r_read)
                _saw("pairs_suppressed" if flags & 48 and not hits else "pairs_over_the_cap" if flags & 48 else "pairs_multi" if flags & 12 else "pairs_one" if flags & 3 else "pairs_none")
            else:                                               # :2565-2585
                if lhits:
                    singleton(obs, L, lidx, left_file, "L", l_proc, l_read)
                else:
                    l_proc.write_unmapped(l_read)
                    stats["num_unmapped_left"] += 1
                    _saw("side_empty_after_exclusion")
                if rhits:
                    singleton(obs, R, ridx, right_file, "R", r_proc, r_read)
                else:
                    r_proc.write_unmapped(r_read)
                    stats["num_unmapped_right"] += 1
                    _saw("side_empty_after_exclusion")
            li += 1
            ri += 1
    left_file.get(VMAX, l_proc)                                 # :2599-2604
    if PE:
        right_file.get(VMAX, r_proc)
        assert lists == {numbers[k]: v for k, v in ch["lists"].items()}, "the walk and pair_ref.choose disagree about the reported pairs"
    return left_out, right_out, [stats[k] for k in STATS]


def pct(num, den):
    """printf("%4.1f") of (100.0 * num) / den as C computes it: a division by zero gives nan or inf, printed as glibc prints them"""
    num = 100.0 * num
    if den == 0:
        return "-nan" if num == 0 else " inf"                   # (0.0 / 0.0 is x86's default NaN, whose sign bit is set: glibc prints "-nan")
    return "%4.1f" % (num / den)


def align_summary(stats, max_multihits):
    """print_alnStats, :2119-2195"""
    s = dict(zip(STATS, stats))
    out = []
    total_left = s["num_aligned_left"] + s["num_unmapped_left"]
    total_right = s["num_aligned_right"] + s["num_unmapped_right"]
    total_unpaired = s["num_aligned_unpaired"] + s["num_unmapped_unpaired"]

    def block(title, total, al, multi, xmulti):
        out.append("%s:\n" % title)
        out.append("          Input     : %9d\n" % total)
        out.append("           Mapped   : %9d (%s%% of input)\n" % (al, pct(al, total)))
        if al and multi > 0:
            out.append("            of these: %9d (%s%%) have multiple alignments (%d have >%d)\n" % (multi, pct(multi, al), xmulti, max_multihits))

    block("Reads" if total_right == 0 else "Left reads", total_left, s["num_aligned_left"], s["num_aligned_left_multi"], s["num_aligned_left_xmulti"])
    total_mapped, total_input, total_pairs = s["num_aligned_left"], total_left, 0
    if total_right:
        block("Right reads", total_right, s["num_aligned_right"], s["num_aligned_right_multi"], s["num_aligned_right_xmulti"])
        total_input += total_right
        total_mapped += s["num_aligned_right"]
        total_pairs = min(total_right, total_left)
        if total_unpaired:
            block("Unpaired reads", total_unpaired, s["num_aligned_unpaired"], s["num_aligned_unpaired_multi"], s["num_aligned_unpaired_xmulti"])
            total_input += total_unpaired
            total_mapped += s["num_aligned_unpaired"]
    out.append("%s%% overall read mapping rate.\n" % pct(total_mapped, total_input))
    if s["num_aligned_pairs"]:
        out.append("\nAligned pairs: %9d\n" % s["num_aligned_pairs"])
        if s["num_aligned_pairs_multi"] > 0:
            out.append("     of these: %9d (%s%%) have multiple alignments\n" % (s["num_aligned_pairs_multi"], pct(s["num_aligned_pairs_multi"], s["num_aligned_pairs"])))
        if s["num_aligned_pairs_disc"] > 0:
            out.append("               %9d (%s%%) are discordant alignments\n" % (s["num_aligned_pairs_disc"], pct(s["num_aligned_pairs_disc"], s["num_aligned_pairs"])))
        out.append("%s%% concordant pair alignment rate.\n" % pct(s["num_aligned_pairs"] - s["num_aligned_pairs_disc"], total_pairs))
    return "".join(out)
