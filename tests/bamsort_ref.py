"""Test-only restatement of what `samtools sort` (0.1.18, by position) does to a file's records, as its loop runs -- not the closed form the
library computes (tophat_amd/csrc/thj_bamsort_core.h): the block cut of bam_sort_core_ext (bam_sort.c:371-381, :384-388), ks_mergesort as
ksort.h:71-118 walks it (its pair step, its `n < i + step` branch) under bam1_lt (bam_sort.c:302-308), and bam_merge_core's heap
(bam_sort.c:202-240) as a repeated choice of the least head under __pos_cmp (:41) with its block number i and its running counter idx.
A record is (tid, pos, strand, size): size = 4 + block_size, what bam_read1 returns."""
import struct

M64 = (1 << 64) - 1
HEAP_EMPTY = M64


def _i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x & 0x80000000 else x


def _sext64(x):
    """an int32 converted to uint64_t"""
    return _i32(x) & M64


def block_key(tid, pos):
    """(uint64_t)a->core.tid << 32 | (a->core.pos + 1): the int32 sum is converted to uint64_t by the usual arithmetic conversions"""
    return ((_sext64(tid) << 32) & M64) | _sext64(_i32(pos + 1))


def merge_key(tid, pos, strand):
    """(uint64_t)tid << 32 | (uint32_t)((int32_t)pos + 1) << 1 | strand: the shift is done in 32 bits"""
    return ((_sext64(tid) << 32) & M64) | (((_i32(pos + 1) & 0xFFFFFFFF) << 1) & 0xFFFFFFFF) | strand


def cut_blocks(sizes, max_mem):
    """-> (blocks as lists of record numbers, merged?): mem += ret; a block ends with the record that makes mem >= max_mem"""
    blocks, cur, mem = [], [], 0
    for i, s in enumerate(sizes):
        cur.append(i)
        mem += s
        if mem >= max_mem:
            blocks.append(cur)
            cur, mem = [], 0
    if not blocks:
        return [cur], False
    blocks.append(cur)                # sort_blocks(n++, k, ...) with what is left, k = 0 included
    return blocks, True


def ks_mergesort(array, lt):
    """ksort.h:71-118, bottom-up, between two arrays"""
    n = len(array)
    a2 = [list(array), [None] * n]
    curr, shift = 0, 0
    while (1 << shift) < n:
        a, b = a2[curr], a2[1 - curr]
        if shift == 0:
            p = 0
            for i in range(0, n, 2):
                if i == n - 1:
                    b[p] = a[i]; p += 1
                elif lt(a[i + 1], a[i]):
                    b[p] = a[i + 1]; b[p + 1] = a[i]; p += 2
                else:
                    b[p] = a[i]; b[p + 1] = a[i + 1]; p += 2
        else:
            step = 1 << shift
            for i in range(0, n, step << 1):
                if n < i + step:
                    ea, eb = n, 0
                else:
                    ea, eb = i + step, min(n, i + (step << 1))
                j, k, p = i, i + step, i
                while j < ea and k < eb:
                    if lt(a[k], a[j]):
                        b[p] = a[k]; k += 1
                    else:
                        b[p] = a[j]; j += 1
                    p += 1
                while j < ea:
                    b[p] = a[j]; j += 1; p += 1
                while k < eb:
                    b[p] = a[k]; k += 1; p += 1
        curr = 1 - curr
        shift += 1
    return a2[curr]


def pos_cmp(a, b):
    """__pos_cmp(a, b): a comes AFTER b; a head is (pos, i, idx)"""
    return a[0] > b[0] or (a[0] == b[0] and (a[1] > b[1] or (a[1] == b[1] and a[2] > b[2])))


def merge(recs, blocks):
    """bam_merge_core: heads, the least of them out, the next record of its block in"""
    at = [0] * len(blocks)
    heads, idx = [], 0
    for i, b in enumerate(blocks):
        if b:
            r = recs[b[0]]
            heads.append([merge_key(r[0], r[1], r[2]), i, idx]); idx += 1
            at[i] = 1
        else:
            heads.append([HEAP_EMPTY, i, 0])
    out = []
    while True:
        least = heads[0]
        for h in heads[1:]:
            if pos_cmp(least, h):
                least = h
        if least[0] == HEAP_EMPTY:
            return out
        i = least[1]
        out.append(blocks[i][at[i] - 1])
        if at[i] < len(blocks[i]):
            r = recs[blocks[i][at[i]]]
            least[0], least[2] = merge_key(r[0], r[1], r[2]), idx
            idx += 1; at[i] += 1
        else:
            least[0] = HEAP_EMPTY


def order(recs, max_mem):
    """-> (the record numbers in output order, how many blocks were written)"""
    blocks, merged = cut_blocks([r[3] for r in recs], max_mem)
    lt = lambda x, y: block_key(recs[x][0], recs[x][1]) < block_key(recs[y][0], recs[y][1])
    blocks = [ks_mergesort(b, lt) for b in blocks]
    if not merged:
        return blocks[0], 1
    return merge(recs, blocks), len(blocks)


def plain_order(recs):
    """the plain stable sort by (tid, pos) a reader might expect: what the fixtures must differ from"""
    return sorted(range(len(recs)), key=lambda i: block_key(recs[i][0], recs[i][1]))


# ---- records as bytes

def make_record(tid, pos, strand, size, qname=b"", fill=0):
    """a BAM record of `size` bytes, block_size field included: QNAME, no cigar, no bases, the rest filler bytes -- the sort reads
    block_size, refID, pos and FLAG only and moves the rest; the filler differs per record so that a misplaced byte shows.  The least
    size is 37: the fixed fields and an empty QNAME's NUL"""
    assert size >= 36 + len(qname) + 1, size
    head = struct.pack("<iiiIIiiii", size - 4, tid, pos, (4680 << 16) | (255 << 8) | (len(qname) + 1), (0x10 if strand else 0) << 16, 0, -1, -1, 0)
    body = bytes((fill * 131 + k * 7 + 1) & 0xFF for k in range(size - 36 - len(qname) - 1))
    return head + qname + b"\x00" + body


def records_bytes(recs):
    """the bytes of (tid, pos, strand, size) rows: QNAME q<number> where it fits, the number as the filler's seed"""
    out = []
    for i, (tid, pos, strand, size) in enumerate(recs):
        q = b"q%d" % i
        out.append(make_record(tid, pos, strand, size, q if size >= 37 + len(q) else b"", fill=i))
    return out


def parse_head(rec):
    """(tid, pos, strand, size) of a record's bytes"""
    bs, tid, pos, _b, fn = struct.unpack_from("<iiiII", rec, 0)
    return tid, pos, 1 if (fn >> 16) & 0x10 else 0, bs + 4


def split_records(stream):
    out, at = [], 0
    while at < len(stream):
        bs = struct.unpack_from("<i", stream, at)[0]
        out.append(stream[at:at + 4 + bs]); at += 4 + bs
    assert at == len(stream)
    return out
