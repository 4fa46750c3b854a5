"""The restatement of the paired-end SAM text (tests/samtext_pe_ref.py) pinned to the reference:
the restated chain (tests/sampe_chain.restated: regions -> sort_and_dedup -> pestat -> rescue ->
mark_primary_se -> pair -> the printed regions -> reg2aln) printed by pair_text equals the
reference's SAM byte for byte -- every line, supplementary ones included -- on
tests/golden/sampe/sampe and the pairing sets rep and rep_a2, except the pairs the chain leaves
to the host, which are pinned by number.  The fixture's classes of lines are asserted from the
committed files, and TLEN is worked by hand.

What the reference's SAM cannot show rests on the reading of software/bwamem.c:1219-1260 alone:
p0 == p1 (no generated pair has equal 5' ends), RG:Z, comments, 0x100 and 0x10000 records
(ref_harness mem has no switch for them).
"""
import gzip
import os

import numpy as np
import pytest

from tests import pair_chain as PC, sampe_chain as SC, samtext_pe_ref as R


@pytest.mark.parametrize("name", SC.SETS)
def test_restated_chain_gives_the_reference_sam(name):
    F = SC.load(name)
    got = SC.texts(F, SC.restated(F))
    n_pairs = F["man"]["pairs"]
    assert len(got) == 2 * n_pairs == len(F["want"])
    host = [p for p in range(n_pairs) if got[2 * p] is None]
    assert host == SC.HOST_PAIRS[name] and len(host) <= PC.MAX_HOST_FRACTION * n_pairs
    n_lines = 0
    for r, w in enumerate(F["want"]):
        if r >> 1 in host:
            assert got[r] is None
            continue
        assert got[r] == w, (name, r, got[r], w)
        n_lines += w.count(b"\n")
    assert n_lines >= 2 * (n_pairs - len(host))
    if name == "sampe":
        assert n_lines == F["man"]["sam_lines"] and F["man"]["left_to_host"] == host


def test_fixture_classes():
    """the committed SAM holds at least ten lines of every class, as its manifest records"""
    F = SC.load("sampe")
    with gzip.open(os.path.join(SC.SAMPE, "sampe.sam.gz"), "rb") as fh:
        cls = SC.classes(fh.read())
    assert cls == F["man"]["classes"] and set(cls) == set(SC.CLASSES)
    assert all(v >= SC.MIN_CLASS for v in cls.values()), cls
    assert sum(F["man"]["kinds"].values()) == F["man"]["pairs"] and abs(F["man"]["pairs"] - 300) <= 30
    assert len({len(x) for x in F["names"]}) >= 15 and all(len(set(q.tolist())) > 10 for q in F["quals"])
    assert all(F["names"][2 * p] == F["names"][2 * p + 1] for p in range(F["man"]["pairs"]))
    # the flags each kind of pair was built for, in the reference's own lines
    flags = {int(line.split(b"\t")[1]) for w in F["want"] for line in w.split(b"\n")[:-1]}
    assert flags >= {99, 147, 83, 163, 73, 133, 117, 185, 77, 141, 97, 145, 67, 131}, sorted(flags)


# ------------------------------------------------------------------ TLEN by hand
def _rec(pos, is_rev, cigar, rid=0):
    return R.Rec(rid=rid, pos=pos, is_rev=is_rev, cigar=tuple(n << 4 | "MIDS".index(op) for n, op in cigar), NM=0, md="0",
                 mapq=60, score=50, xs=0)


def test_get_rlen_counts_m_and_d():
    assert R.get_rlen(_rec(0, 0, [(5, "S"), (20, "M"), (3, "I"), (10, "M"), (4, "D"), (12, "M"), (7, "S")]).cigar) == 46
    assert R.get_rlen(()) == 0


@pytest.mark.parametrize("p,m,want", [
    # forward read at 100, reverse mate whose last base is 100 + 299: the fragment's 300 bases, and its mirror
    (_rec(100, 0, [(50, "M")]), _rec(350, 1, [(50, "M")]), 300),
    (_rec(350, 1, [(50, "M")]), _rec(100, 0, [(50, "M")]), -300),
    # p0 == p1: a forward read at the base a reverse mate ends on -- and two forward reads at one place
    (_rec(149, 0, [(50, "M")]), _rec(100, 1, [(50, "M")]), 0),
    (_rec(100, 0, [(50, "M")]), _rec(100, 0, [(30, "M")]), 0),
    # neighbours: one base apart is +-2
    (_rec(100, 0, [(50, "M")]), _rec(101, 0, [(50, "M")]), 2),
    (_rec(101, 0, [(50, "M")]), _rec(100, 0, [(50, "M")]), -2),
    # a reverse read with clips, an insertion and a deletion: 5S20M3I10M4D12M7S spans 20 + 10 + 4 + 12 = 46 reference
    # bases, its 5' end is 1000 + 45; the forward mate at 800: p0 - p1 = 245, TLEN -(245 + 1)
    (_rec(1000, 1, [(5, "S"), (20, "M"), (3, "I"), (10, "M"), (4, "D"), (12, "M"), (7, "S")]), _rec(800, 0, [(57, "M")]), -246),
    (_rec(800, 0, [(57, "M")]), _rec(1000, 1, [(5, "S"), (20, "M"), (3, "I"), (10, "M"), (4, "D"), (12, "M"), (7, "S")]), 246),
    # either side without a CIGAR: 0
    (_rec(100, 0, []), _rec(350, 1, [(50, "M")]), 0),
    (_rec(100, 0, [(50, "M")]), _rec(350, 1, []), 0),
])
def test_tlen_by_hand(p, m, want):
    assert R.tlen(p, m) == want


def test_lines_by_hand():
    """flags, both copy rules, RNEXT / PNEXT / TLEN and the reverse-complemented placed read, each
    line written out by hand from software/bwamem.c:1219-1260"""
    c = np.array([0, 1, 2, 3, 0, 1], dtype=np.uint8)                       # ACGTAC
    q = np.frombuffer(b"ABCDEF", dtype=np.uint8)
    names, offs = ["chr1", "chr2"], [0, 1000]
    fwd = R.Rec(rid=0, pos=99, is_rev=0, cigar=(6 << 4,), NM=0, md="6", mapq=60, score=6, xs=0)
    rev = R.Rec(rid=0, pos=299, is_rev=1, cigar=(2 << 4 | 3, 2 << 4, 1 << 4 | 1, 3 << 4 | 2, 1 << 4), NM=4, md="2^AAA1", mapq=50,
                score=3, xs=-1)
    read = lambda recs: dict(name="x", codes=c, qual=q, comment="", recs=recs)   # noqa: E731
    sel = lambda branch, proper, mapq=(-1, -1): dict(status=0, branch=branch, proper=proper, mapq=list(mapq))   # noqa: E731
    # branch 1: 0x40 / 0x80 | 3, the pair's MAPQ; rev spans 2M3D1M = 6 bases: p1 = 299 + 5, TLEN 304 - 99 + 1
    assert R.pair_text([read([fwd]), read([rev])], sel(1, 1, (33, 44)), names, offs) == [
        b"x\t99\tchr1\t100\t33\t6M\t=\t300\t206\tACGTAC\tABCDEF\tNM:i:0\tMD:Z:6\tAS:i:6\tXS:i:0\n",
        b"x\t147\tchr1\t300\t44\t2S2M1I3D1M\t=\t100\t-206\tGTACGT\tFEDCBA\tNM:i:4\tMD:Z:2^AAA1\tAS:i:3\n"]
    # branch 0, an unmapped second end: 0x8 and the read's own place on the first; RNAME / POS / 0 / * on the second
    assert R.pair_text([read([fwd]), read([])], sel(0, 1), names, offs) == [
        b"x\t73\tchr1\t100\t60\t6M\t=\t100\t0\tACGTAC\tABCDEF\tNM:i:0\tMD:Z:6\tAS:i:6\tXS:i:0\n",
        b"x\t133\tchr1\t100\t0\t*\t=\t100\t0\tACGTAC\tABCDEF\tAS:i:0\tXS:i:0\n"]
    # ... on a reverse mate: 0x20 from its own strand on the mapped read; 0x10 | 0x20 and SEQ / QUAL turned on the placed one
    fr = R.replace(fwd, is_rev=1)
    assert R.pair_text([read([]), read([fr])], sel(0, 0), names, offs) == [
        b"x\t117\tchr1\t100\t0\t*\t=\t100\t0\tGTACGT\tFEDCBA\tAS:i:0\tXS:i:0\n",
        b"x\t185\tchr1\t100\t60\t6M\t=\t100\t0\tGTACGT\tFEDCBA\tNM:i:0\tMD:Z:6\tAS:i:6\tXS:i:0\n"]
    # both unmapped
    assert R.pair_text([read([]), read([])], sel(0, 1), names, offs) == [
        b"x\t77\t*\t0\t0\t*\t*\t0\t0\tACGTAC\tABCDEF\tAS:i:0\tXS:i:0\n",
        b"x\t141\t*\t0\t0\t*\t*\t0\t0\tACGTAC\tABCDEF\tAS:i:0\tXS:i:0\n"]
    # across contigs: RNEXT a name, TLEN 0, and proper = 1 does not reach the flag in branch 0 (:321)
    other = R.replace(rev, rid=1, pos=1000 + 41)
    assert R.pair_text([read([fwd]), read([other])], sel(0, 1), names, offs) == [
        b"x\t97\tchr1\t100\t60\t6M\tchr2\t42\t0\tACGTAC\tABCDEF\tNM:i:0\tMD:Z:6\tAS:i:6\tXS:i:0\n",
        b"x\t145\tchr2\t42\t50\t2S2M1I3D1M\tchr1\t100\t0\tGTACGT\tFEDCBA\tNM:i:4\tMD:Z:2^AAA1\tAS:i:3\n"]
    # a supplementary line is printed against the same mate with its own RNAME and POS
    sup = R.replace(other, flag=0x800, mapq=7, xs=1)
    t = R.pair_text([read([fwd, sup]), read([rev])], sel(0, 1), names, offs)
    assert t[0].split(b"\n")[1] == (b"x\t2163\tchr2\t42\t7\t2H2M1I3D1M\tchr1\t300\t0\tACGT\tDCBA\tNM:i:4\tMD:Z:2^AAA1\tAS:i:3\tXS:i:1"
                                    b"\tSA:Z:chr1,100,+,6M,60,0;")
    assert t[1] == b"x\t147\tchr1\t300\t50\t2S2M1I3D1M\t=\t100\t-206\tGTACGT\tFEDCBA\tNM:i:4\tMD:Z:2^AAA1\tAS:i:3\n"
    # the host's pair
    assert R.pair_text([read([fwd]), read([rev])], dict(sel(1, 1, (1, 2)), status=1), names, offs) is None
    assert R.pair_text([read([fwd]), read([R.replace(rev, status=3)])], sel(0, 0), names, offs) is None
