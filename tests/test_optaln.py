"""Raw regions -> final regions -> alignments under non-default `bwa mem`
options and on reads of up to 1 kbp, without a GPU: the restatements
(tests/regfin_ref.py, tests/reg2aln_ref.py) against the reference's own records
of the r3 / r4 reads under nine option sets (tests/golden/optaln/, made by
tests/golden/make_golden_optaln.py over the raw regions committed with the
chains -> regions tests), and what those regions reach in the GPU stage, judged
by the restated classifier (reg2aln_ref.classify).

Bar: exact.  tests/test_gpu_optaln.py then holds the GPU to the same records
and to these restatements.
"""
import re

import pytest

import optaln_data as O
import reg2aln_ref as ref
import regfin_data as D


@pytest.mark.parametrize("name", O.SETS)
def test_reg2aln_restatement_vs_reference_records(name):
    """Every record of the reference that has a raw region of its geometry equals
    reg2aln_ref.reg2aln of that region under the set's scoring in (is_rev, pos, CIGAR with
    clips, NM, MD), no tolerance; at most 2 % of the records find no region; the manifest's
    counts are what is counted here."""
    F = O.load(name)
    n = n_un = gapped = 0
    for r, recs in enumerate(F["records"]):
        for w, h in zip(recs or [], F["hits"][r]):
            n += 1
            if h < 0:
                n_un += 1
                continue
            a = O.align(name, r, F["regs"][h])
            assert a.status == 0
            assert (a.is_rev, a.pos, a.cigar, a.NM, a.md) == O.record_tuple(F, w), (r, w, a)
            gapped += bool(re.search("[ID]", w["cigar"]))
    print(f"{name}: {n} records, {n_un} without a region, {gapped} matched with a gap")
    assert n_un <= O.MAX_UNMATCHED * n, (n_un, n)
    man = F["man"]
    assert (n, n - n_un, gapped) == (man["records"], man["matched"], man["matched_gapped"])
    assert man["reads_kept"] == sum(1 for recs in F["records"] if recs is not None)


@pytest.mark.parametrize("name", O.SETS)
def test_finalize_restatement_vs_reference_records(name):
    """Every read's records equal predict_records(finalize(...)) under the set's options
    (T = 30 a) in number, flag, MAPQ, AS and XS, and in contig and position where the region
    does not bridge two contigs."""
    F = O.load(name)
    for r, (a, sel, idx) in enumerate(O.fin_rows(name)):
        want = F["records"][r]
        if want is None:
            continue
        got = D.predict_records(F, r, a, sel, idx)
        assert len(got) == len(want), (r, got, want)
        for g, w in zip(got, want):
            assert all(g[k] == w[k] for k in ("flag", "mapq", "AS", "XS")), (r, g, w)
            assert g["pos"] is None or (g["rname"], g["pos"]) == (w["rname"], w["pos"]), (r, g, w)


def test_fixture_regions_reach_the_kernel_paths():
    """Over the selected final regions of the sets (what the resident chain aligns): every
    class of g2a_prep_kernel, at least 100 scratch-tier regions in one set, tries of 2 and
    of 3, a deferral from the 16-lane and from the 32-lane class, and a retry run in a lane
    group's LDS on more columns than the group has lanes (the multi-pass carry)."""
    cov = {}
    for name in O.SETS:
        cov[name] = c = O.coverage(name, [(p, a) for row in O.expected(name) for p, a, _rid in row])
        print(name, c)
    for cls in range(4):
        assert any(c["classes"][cls] for c in cov.values()), cls
    assert max(c["classes"][ref.SCRATCH_CLASS] for c in cov.values()) >= 100
    assert any(c["tries"].get(2) for c in cov.values()) and any(c["tries"].get(3) for c in cov.values())
    assert any(c["deferred"].get(0) for c in cov.values()) and any(c["deferred"].get(1) for c in cov.values())
    assert any(c["lds_retry_wide"] for c in cov.values())
    # the figures the fixtures were chosen for
    assert cov["g1_r3_default"]["classes"] == [354, 33, 123, 142]
    assert cov["g1_r3_w7"]["tries"] == {1: 724, 2: 6, 3: 2} and cov["g1_r3_w7"]["deferred"] == {0: 5}
    assert cov["g2_r4_w7"]["deferred"] == {1: 1}
    assert all(c["tries"].keys() == {1} for n, c in cov.items() if n.endswith("default"))
