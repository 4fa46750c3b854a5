"""Raw regions -> final list, primary marks, selection, MAPQ and flags
(mem_sort_and_dedup, mem_mark_primary_se and the head of mem_reg2sam_se /
mem_reg2aln, software/bwamem.c:705-785, 1333-1379): the Python restatement
(tests/regfin_ref.py) pinned, without a GPU, to the reference's own files --
its regions (SMRG) and the SAM records it printed from them.

Bar: exact, no read left out.  mem_test_and_remove_exact after a
de-duplication is reached by no command of the committed reference harness,
so the NO_EXACT flag is checked against the restatement's reading of its three
lines only (here and in tests/test_gpu_regfin.py).
"""
import math

import numpy as np
import pytest

import regfin_data as D
import regfin_ref as ref


def _compare(name, keys):
    F = D.load(name)
    out, _ = D.restated(name)
    n_reads = n_rec = n_pos_exempt = 0
    bad = []
    for r, (a, sel, idx) in enumerate(out):
        want = F["records"][r]
        if want is None:       # under 30 bp: not in the reference's FASTQ
            continue
        n_reads += 1
        got = D.predict_records(F, r, a, sel, idx)
        ok = len(got) == len(want)
        for g, w in zip(got, want):
            ok = ok and all(g[k] == w[k] for k in keys)
            if g["pos"] is None:
                n_pos_exempt += 1
            else:
                ok = ok and (g["rname"], g["pos"]) == (w["rname"], w["pos"])
        n_rec += len(want)
        if not ok:
            bad.append((r, got, want))
    return n_reads, n_rec, n_pos_exempt, bad


@pytest.mark.parametrize("name,reads,records,exempt", [("g1_default_std", 1417, 1302, 1),
                                                       ("g2_default_std", 494, 492, 1)])
def test_restatement_vs_reference_sam(name, reads, records, exempt):
    """(a) every read of the reference's single-end run: its mapped records equal the
    prediction in count, order, flag, MAPQ, AS, XS and position; the hash id is the
    read's ordinal in the FASTQ.  Only a region bridging a contig boundary is exempt
    from the position (bwa_fix_xref2 moves or trims it): r401 of g1, r171 of g2."""
    n_reads, n_rec, n_exempt, bad = _compare(name, ("flag", "mapq", "AS", "XS"))
    assert (n_reads, n_rec) == (reads, records)
    assert not bad, f"{len(bad)} reads differ, the first: {bad[0]}"
    assert n_exempt == exempt


@pytest.mark.parametrize("name,reads,records", [("cigar_g1", 370, 377), ("cigar_g2", 370, 379), ("g2_r4", 283, 342)])
def test_restatement_vs_reference_cigar_records(name, reads, records):
    """(b) the gapped reads and the long reads of r4: flag, order and position of every
    record, id = read index; and, from tests/golden/regfin/, MAPQ, AS and XS -- on the long
    reads the cap of a supplementary record's MAPQ at the first record's"""
    n_reads, n_rec, _n_exempt, bad = _compare(name, ("flag", "mapq", "AS", "XS"))
    assert n_reads == reads and n_rec == records
    assert not bad, f"{len(bad)} reads differ, the first: {bad[0]}"
    if name == "cigar_g2":
        out, _ = D.restated(name)
        assert sum(1 for a, _, _ in out for p in a if p["secondary"] >= 0) == 264


def test_fixtures_bite():
    """(c) the fixtures reach what makes the stage hard"""
    big = eq_re = comb = removed = xs = 0
    mapqs = set()
    for name in ("g1_default_std", "g2_default_std"):
        F = D.load(name)
        out, ctr = D.restated(name)
        comb += ctr.combsort
        for r, (a, sel, idx) in enumerate(out):
            lo, hi = int(F["reg_off"][r]), int(F["reg_off"][r + 1])
            big += hi - lo > 16
            eq_re += np.unique(F["regs"]["re"][lo:hi]).size < hi - lo
            removed += hi - lo - len(a)
            for w in F["records"][r] or []:
                xs += (w["XS"] or 0) > 0
                if name[:2] == "g2":
                    mapqs.add(w["mapq"])
    assert big > 0 and eq_re > 0 and comb > 0 and xs > 0
    assert removed == 303 + 526
    assert len(mapqs) == 38


def test_supplementary_records_present():
    n = sum(1 for name in ("cigar_g1", "cigar_g2") for recs in D.load(name)["records"] for w in recs
            if w["flag"] & 0x800)
    assert n == 19
    # r4: supplementary records whose own MAPQ would be higher than the first record's
    out, _ = D.restated("g2_r4")
    capped = 0
    for a, sel, idx in out:
        for k in idx[1:]:
            if a[k]["secondary"] < 0 and ref.approx_mapq_se(ref.Opt(), a[k]) > sel[k][0]:
                capped += 1
    assert capped > 0


# ------------------------------------------------- the restatement's own parts
def test_introsort_sorts_and_is_not_stable():
    rng = np.random.default_rng(3)
    unstable = 0
    for n in list(range(0, 40)) + [63, 64, 65, 129, 300, 1000]:
        keys = rng.integers(0, 6, n).tolist()
        a = [(k, i) for i, k in enumerate(keys)]
        ref.ks_introsort(a, lambda x, y: x[0] < y[0])
        assert [k for k, _ in a] == sorted(keys)
        unstable += a != sorted(a)
    assert unstable > 0
    ctr = ref.Counters()
    a = [(i // 4, i) for i in range(100)]   # ascending input with equal keys uses up the depth budget
    ref.ks_introsort(a, lambda x, y: x[0] < y[0], ctr)
    assert ctr.combsort > 0 and [k for k, _ in a] == [i // 4 for i in range(100)]


def test_hash_64():
    """a bijection of 64-bit keys (its value is pinned by the order of equal scores in (a))"""
    seen = {ref.hash_64(i) for i in range(4096)}
    assert len(seen) == 4096 and all(0 <= h < 1 << 64 for h in seen)


def _reg(rb, re_, qb, qe, score, **kw):
    d = dict(rb=rb, re=re_, qb=qb, qe=qe, score=score, truesc=score, sub=0, csub=0, sub_n=0, w=100, seedcov=qe - qb,
             secondary=-1, hash=0)
    d.update(kw)
    return d


def test_float_overlap_cases():
    """19 of 20 is not redundant at 0.95 in float (the product rounds to 19.0), and
    10 of 20 is a significant overlap at 0.5"""
    assert np.float32(0.95) * np.float32(20) == np.float32(19)
    assert float(np.float32(0.95)) * 20 < 19      # the same product in double
    a = ref.sort_and_dedup([_reg(100, 120, 0, 20, 20), _reg(101, 121, 1, 21, 19)], 0.95)
    assert len(a) == 2
    a = ref.sort_and_dedup([_reg(100, 120, 0, 20, 20), _reg(100, 121, 0, 21, 19)], 0.95)
    assert len(a) == 1 and a[0]["score"] == 20
    a = ref.mark_primary_se(ref.Opt(), [_reg(100, 120, 0, 20, 20), _reg(500, 520, 10, 30, 19)], 0)
    assert sorted(p["secondary"] for p in a) == [-1, 0]
    a = ref.mark_primary_se(ref.Opt(), [_reg(100, 120, 0, 20, 20), _reg(500, 520, 11, 31, 19)], 0)
    assert [p["secondary"] for p in a] == [-1, -1]


def test_mapq_coef_fac_is_an_int():
    r = _reg(1000, 1100, 0, 100, 40, seedcov=40)
    # identity 1 - 60 / 5 / 100 = 0.88, score - sub = 21
    want = [int(6.02 * 21 * (f / math.log(100) * 0.88 * 0.88) ** 2 + .499) for f in (3, 3.912)]
    assert want[0] != want[1]
    assert ref.approx_mapq_se(ref.Opt(), r) == want[0]
    assert ref.approx_mapq_se(ref.Opt(mapQ_coef_fac=3.912), r) == want[1]
