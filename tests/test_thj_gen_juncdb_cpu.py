"""CPU: `thj_gen --juncdb` (bench / test infrastructure): the option adds the junction-db segment maps and changes no other file, and
every record it writes is a segment the spliced hit factory turns into a hit across its gene's planted junction."""
import hashlib
import os
import re
import subprocess

import pytest

from tophat_amd.samtext import parse_spliced_sam_hits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gen():
    exe = os.path.join(ROOT, "tools", "bin", "thj_gen")
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    return exe


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def test_juncdb_option_adds_maps_and_changes_nothing_else(gen, tmp_path):
    a, b = str(tmp_path / "plain"), str(tmp_path / "juncdb")
    common = ["--pairs", "3000", "--genome-len", "3000000", "--introns", "300", "--indel-frac", "0.03", "--text", "--threads", "3"]
    subprocess.check_call([gen, "--out", a] + common, stdout=subprocess.DEVNULL)
    subprocess.check_call([gen, "--out", b] + common + ["--juncdb"], stdout=subprocess.DEVNULL)
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert not [f for f in fa if "to_spliced" in f]
    assert [f for f in fb if "to_spliced" not in f] == fa
    for f in fa:
        assert sha(os.path.join(a, f)) == sha(os.path.join(b, f)), f
    extra = [f for f in fb if "to_spliced" in f]
    assert sorted(extra) == sorted("%s_seg%d.to_spliced.%s" % (sd, k, e) for sd in ("left", "right") for k in (1, 2, 3, 4) for e in ("bam", "bam.index", "sam"))
    # every record: a plain M against `contig|left_start|l-r|right_end|GTAG|fwd|rev`, spliced by the factory into aM gN bM over (l, r)
    n = 0
    for sd in ("left", "right"):
        for k in (1, 2, 3, 4):
            sam = os.path.join(b, "%s_seg%d.to_spliced.sam" % (sd, k))
            lines = [l.split("\t") for l in open(sam) if not l.startswith("@")]
            hits = list(parse_spliced_sam_hits(sam, {"chr20": 1}))
            assert len(hits) == len(lines), "the factory keeps every record"
            for f, h in zip(lines, hits):
                m = re.fullmatch(r"chr20\|(\d+)\|(\d+)-(\d+)\|(\d+)\|GTAG\|(fwd|rev)", f[2])
                assert m and int(m.group(2)) - int(m.group(1)) + 1 == 100 and int(m.group(4)) - int(m.group(3)) == 100
                l, r = int(m.group(2)), int(m.group(3))
                (o0, n0), (o1, n1), (o2, n2) = h[9]
                assert (o0, o1, o2) == (1, 11, 1) and n0 > 3 and n2 > 3 and n0 + n2 == len(f[9]) and n1 == r - l - 1
                assert h[2] + n0 == l + 1 and h[6] <= 2 and h[10] == (m.group(5) == "rev")
                assert int(f[0].split("|")[0]) == h[0] and re.fullmatch(r"\d+\|%d:%d:4" % (25 * (k - 1), k - 1), f[0])
                n += 1
    assert n > 500
