#!/usr/bin/env python3
"""Mints tests/golden/samtools_sort/* with REFERENCE code: the reference's vendored samtools 0.1.18 (plain C + zlib), compiled from the
sources where they lie under /root/reference into a temporary directory outside the repository, together with a two-line driver of
ours that calls its bam_sort (the body of `samtools sort`).  Build container only; nothing of the tool is kept, only what it did:

  <case>.json     {"max_mem": the -m value, "records": [[tid, pos, strand, size], ...] in input order,
                   "order": the input record numbers in the order the reference's output file holds them}
  MANIFEST.json   per case: records, blocks written (counted from the block cut), whether the recorded order differs from the plain
                  stable sort by (tid, pos), the sha256 of the case file

The input BAM of a case holds tests/bamsort_ref.py's records_bytes() of the rows (QNAME q<number>), so a test rebuilds the same bytes from
the rows; the output order is read back from the QNAMEs.  -m stays >= 2000: the reference's buffer has max_mem / 32 slots.  At least
two cases must differ from the plain stable sort (mixed strands at one position in two blocks, reverse before forward inside a
block) -- checked here and again in tests/test_bamsort_cpu.py: without it the fixtures pin nothing that sorted() does not.

    python tests/golden/samtools_sort/mint.py        (needs /root/reference; rewrites the directory's data files)"""
import gzip
import hashlib
import json
import os
import random
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import bamsort_ref as bs                                    # noqa: E402
from ingest_cases import bam_header, bgzf_member            # noqa: E402

REF = "/root/reference/src/samtools-0.1.18"
SRC = "bgzf kstring bam_aux bam bam_import sam sam_header razf faidx knetfile bam_md kprobaln bam_pileup bam_index bam_sort".split()
DRIVER = "int bam_sort(int argc, char *argv[]);\nint main(int argc, char *argv[]) { return bam_sort(argc, argv); }\n"
TARGETS = (("chrA", 100000), ("chrB", 100000), ("chrC", 100000), ("chrD", 100000))


def cases():
    out = {}
    r = random.Random(20260101)
    out["mixed_strands_a"] = (2000, [(r.randrange(3), r.randrange(6), r.randrange(2), r.randrange(60, 121)) for _ in range(300)])
    out["mixed_strands_b"] = (3000, [(r.randrange(2), r.choice((10, 10, 10, 11, 500)), r.randrange(2), r.randrange(40, 301)) for _ in range(400)])
    out["mixed_strands_c"] = (2048, [(0, r.randrange(3), int(r.random() < 0.3), r.choice((64, 100, 128))) for _ in range(256)])
    out["one_block"] = (1000000000, [(r.randrange(3), r.randrange(6), r.randrange(2), r.randrange(60, 121)) for _ in range(300)])
    out["cut_at_the_last_record"] = (2000, [(r.randrange(2), r.randrange(4), r.randrange(2), 100) for _ in range(200)])
    out["unmapped_among_mapped"] = (2500, [(-1, -1, r.randrange(2), r.randrange(50, 90)) if r.random() < 0.3 else (r.randrange(4), r.randrange(-1, 3), r.randrange(2), r.randrange(50, 90))
                                           for _ in range(300)])
    out["distinct_positions_falling"] = (2200, [(1 - k // 150, 5000 - 7 * k, k % 2, 70 + k % 13) for k in range(300)])
    return out


def build_tool(tmp):
    open(os.path.join(tmp, "drv.c"), "w").write(DRIVER)
    exe = os.path.join(tmp, "stsort")
    cmd = ["gcc", "-O2", "-w", "-D_FILE_OFFSET_BITS=64", "-D_LARGEFILE64_SOURCE", "-D_USE_KNETFILE", "-I" + REF, os.path.join(tmp, "drv.c")]
    subprocess.check_call(cmd + [os.path.join(REF, s + ".c") for s in SRC] + ["-o", exe, "-lz", "-lm"])
    return exe


def write_input(path, recs):
    data = bam_header(TARGETS, "@HD\tVN:1.0\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % t for t in TARGETS))
    out = bytearray()
    for rec in bs.records_bytes(recs):
        if len(data) + len(rec) > 60000:
            out += bgzf_member(bytes(data)); data = b""
        data += rec
    out += bgzf_member(bytes(data)) + bgzf_member(b"")
    open(path, "wb").write(out)
    return len(bam_header(TARGETS, "@HD\tVN:1.0\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % t for t in TARGETS)))


def main():
    if not os.path.isdir(REF):
        sys.exit("%s is not present" % REF)
    tmp = tempfile.mkdtemp(prefix="thj_mint_sort_")
    manifest = {"made_by": "tests/golden/samtools_sort/mint.py: bam_sort of the reference's samtools 0.1.18 sources, run with -m", "cases": {}}
    try:
        exe = build_tool(tmp)
        differ = 0
        for name, (max_mem, recs) in sorted(cases().items()):
            assert max_mem >= 2000
            src = os.path.join(tmp, name + ".bam")
            hdr_len = write_input(src, recs)
            subprocess.run([exe, "-m", str(max_mem), src, os.path.join(tmp, name + ".sorted")], check=True, stderr=subprocess.DEVNULL)
            stream = gzip.open(os.path.join(tmp, name + ".sorted.bam"), "rb").read()[hdr_len:]
            want = bs.records_bytes(recs)
            number = {w: i for i, w in enumerate(want)}
            assert len(number) == len(want)
            order = [number[g] for g in bs.split_records(stream)]
            assert sorted(order) == list(range(len(recs))), name
            blocks, merged = bs.cut_blocks([x[3] for x in recs], max_mem)
            d = order != bs.plain_order(recs)
            differ += d
            path = os.path.join(HERE, name + ".json")
            with open(path, "w") as f:
                json.dump({"max_mem": max_mem, "records": [list(x) for x in recs], "order": order}, f, separators=(",", ":"))
                f.write("\n")
            manifest["cases"][name] = {"records": len(recs), "blocks": len(blocks) if merged else 1, "differs_from_plain_stable_sort": bool(d),
                                       "sha256": hashlib.sha256(open(path, "rb").read()).hexdigest()}
            print(name, len(recs), "records,", manifest["cases"][name]["blocks"], "blocks, differs from the plain sort:", bool(d))
        assert differ >= 2, "fewer than two cases differ from the plain stable sort: the fixtures would pin nothing"
        with open(os.path.join(HERE, "MANIFEST.json"), "w") as f:
            json.dump(manifest, f, indent=1, sort_keys=True)
            f.write("\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
