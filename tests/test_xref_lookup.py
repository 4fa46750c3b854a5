"""The contig lookup of smem_batch_reg2aln, without a GPU: tests/xref_ref.py
(bns_depos, bns_pos2rid, the "fix is needed" test of bwa_fix_xref2) pinned to
the reference's own records, and the library's new entry points.

For every mapped record of the reference on four fixture sets, the final
region the restatements select for it (tests/regfin_ref.py) is aligned
(tests/reg2aln_ref.py); bns_pos2rid of the alignment's position must name the
record's contig and the position within it must be the record's.  The regions
for which the lookup says bwa_fix_xref2 changes something must be exactly the
ones that bridge a contig boundary.
"""
import ctypes as C
import re

import pytest

import regfin_data as D
import xref_ref as X

SETS = ("g1_default_std", "g2_default_std", "cigar_g1", "cigar_g2")


@pytest.mark.parametrize("name", SETS)
def test_lookup_names_the_reference_records(name):
    F = D.load(name)
    names, offs, lens = X.table(F["contigs"])
    l_pac = F["l_pac"]
    want_rows = X.expected(name)
    n = n_fix = 0
    for r, recs in enumerate(F["records"]):
        if recs is None:
            continue
        row = want_rows[r]
        assert len(row) == len(recs), (r, row, recs)
        for (p, aln, rid), w in zip(row, recs):
            n += 1
            bridging = D.predict_records(F, r, [p], [(0, 0, 0)], [0])[0]["pos"] is None
            assert X.needs_fix(offs, lens, l_pac, p["rb"], p["re"]) == bridging, (r, p)
            if bridging:
                assert aln.status == X.XREF and rid == -1
                n_fix += 1
                continue
            assert aln.status == 0, (r, p, aln)
            assert rid == X.pos2rid(offs, l_pac, aln.pos) and names[rid] == w["rname"], (r, w, aln, rid)
            assert aln.pos - int(offs[rid]) + 1 == w["pos"], (r, w, aln)
    print(f"{name}: {n} records, {n_fix} need bwa_fix_xref2")
    assert n > 300 and n_fix <= 2


def test_each_genome_has_a_bridging_region():
    """r401 of g1 and r171 of g2: the status is reached, nothing is exempted wholesale"""
    for g in ("g1", "g2"):
        got = [(r, k) for r, row in enumerate(X.expected(f"{g}_default_std")) for k, (_p, a, _rid) in enumerate(row)
               if a.status == X.XREF]
        assert 1 <= len(got) <= 2, (g, got)
    assert any(a.status == X.XREF for a in (t[1] for t in X.expected("g1_default_std")[401]))
    assert any(a.status == X.XREF for a in (t[1] for t in X.expected("g2_default_std")[171]))
    # without a table nothing is marked and no contig is named
    for row in X.expected("g1_default_std", with_contigs=False):
        assert all(a.status != X.XREF and rid == -1 for _p, a, rid in row)


def test_search_edge_cases():
    offs, lens, l_pac = [0, 10, 11, 40], [10, 1, 29, 60], 100
    for i, (o, n) in enumerate(zip(offs, lens)):
        assert X.pos2rid(offs, l_pac, o) == i                 # a contig's first base
        assert X.pos2rid(offs, l_pac, o + n - 1) == i         # and its last
    assert X.pos2rid(offs, l_pac, l_pac) == -1 and X.pos2rid(offs, l_pac, l_pac + 5) == -1
    assert [X.pos2rid([0], 7, p) for p in (0, 3, 6, 7)] == [0, 0, 0, -1]       # a one-contig table
    assert X.depos(l_pac, 0) == (0, 0) and X.depos(l_pac, 99) == (99, 0)
    assert X.depos(l_pac, 100) == (99, 1) and X.depos(l_pac, 199) == (0, 1)
    # a region within a contig, up to both of its ends, on either strand; one base over either end
    assert not X.needs_fix(offs, lens, l_pac, 11, 40) and not X.needs_fix(offs, lens, l_pac, 200 - 40, 200 - 11)
    assert X.needs_fix(offs, lens, l_pac, 10, 40) and X.needs_fix(offs, lens, l_pac, 11, 41)
    assert X.needs_fix(offs, lens, l_pac, 200 - 41, 200 - 11) and X.needs_fix(offs, lens, l_pac, 200 - 40, 200 - 10)
    assert not X.needs_fix([0], [7], 7, 0, 7) and not X.needs_fix([0], [7], 7, 7, 14)


def _header_stats_fields():
    """the members of smem_batch_stats_t, with their C types, from include/smem_gpu.h"""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "smem_gpu.h")) as fh:
        text = fh.read()
    body = re.search(r"typedef struct \{([^}]*)\} smem_batch_stats_t;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        m = re.match(r"\s*(double|uint64_t|uint32_t|int)\s+(.*)", decl.strip(), flags=re.S)
        if m:
            out += [(v.strip(), m.group(1)) for v in m.group(2).split(",")]
    return out


def test_library_exports_and_stats_layout(built):
    """the built library has the stage's entry points, the binding's constants and its
    smem_batch_stats_t are the header's"""
    import smemgpu
    from smemgpu import lib
    so = smemgpu.load()
    for fn in ("smem_batch_reg2aln", "smem_gpu_load_contigs", "smem_batch_aln2_results"):
        assert hasattr(so, fn), fn
    assert lib.FETCH_ALN == 32 and lib.ALN_XREF == 4 and not lib.FETCH_ALL & lib.FETCH_ALN
    ctype = {"double": C.c_double, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int": C.c_int}
    want = [(n, ctype[t]) for n, t in _header_stats_fields()]
    assert [(n, t) for n, t in lib.BatchStats._fields_] == want

    class Implied(C.Structure):
        _fields_ = want
    assert C.sizeof(lib.BatchStats) == C.sizeof(Implied)
    assert [n for n, _ in want][-6:] == ["g2a_ms", "g2a_prep_ms", "n_g2a", "n_g2a_deferred", "n_g2a_xref", "n_g2a_passes"]
