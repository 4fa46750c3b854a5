"""Raw regions -> final regions -> alignments on the GPU under non-default
`bwa mem` options and on reads of up to 1 kbp: smem_reg2aln, smem_reg_finalize
and the resident chain (seed, SA, chain, chain2aln, reg_finalize, reg2aln) over
the r3 / r4 reads under nine option sets each (tests/golden/optaln/).

Bar: exact.  Every record equals the reference's own (flag, contig, position,
MAPQ, CIGAR, NM, MD) and the restatements in every field (tests/optaln_data.py;
tests/test_optaln.py pins those to the same records without a GPU).  The
stage's counters equal what the restated classifier (reg2aln_ref.classify)
predicts: these regions reach the scratch tier by the hundred, retry with a
doubled band, run rows of several passes in the 16-lane kernel and defer from
the 16- and the 32-lane class (test_optaln.test_fixture_regions_reach_the_kernel_paths).
"""
import os

import numpy as np
import pytest

import optaln_data as O
import reg2aln_ref
import regfin_data as D
import test_reg2aln as T
import xref_ref as X
from tests import golden_data

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handles(gpu_device, tmp_path_factory):
    """one handle per genome, opened on first use: index, .sa, .pac and contig table resident"""
    import smemgpu
    made = {}

    def get(g):
        if g not in made:
            paths = golden_data.files(g, str(tmp_path_factory.mktemp(g)))
            gpu = smemgpu.Gpu(smemgpu.Index.read(paths["bwt"]), device=gpu_device)
            gpu.load_sa(smemgpu.SA.read(paths["sa"]))
            gpu.load_pac(golden_data.pac(g), golden_data.l_pac(g))
            _n, offs, lens = X.table(D.contigs(g))
            gpu.load_contigs(offs, lens, golden_data.l_pac(g))
            made[g] = gpu
        return made[g]
    yield get
    for gpu in made.values():
        gpu.close()


def _aln_opt(F):
    """smem_aln_opt_t of the set: what chain2aln and reg2aln read"""
    from oracle import oracle
    return oracle.aln_opt(**F["opt"])


def _fin_opt(F):
    import smemgpu
    o = F["fin_opt"]
    return smemgpu.fin_opt(a=o.a, b=o.b, o_del=o.o_del, e_del=o.e_del, o_ins=o.o_ins, e_ins=o.e_ins,
                           min_seed_len=o.min_seed_len, T=o.T)


@pytest.mark.parametrize("name", O.SETS)
def test_host_reg2aln(handles, name):
    """smem_reg2aln over every raw region under the set's scoring: a region with a record of
    the reference equals it in (is_rev, pos, CIGAR with clips, NM, MD), every region equals the
    restatement in every smem_aln_t field, and the pools are exactly used"""
    F = O.load(name)
    want = O.raw_aligned(name)
    alns, cigar, md, ms = handles(F["g"]).reg2aln(None, F["l_pac"], F["reads"].codes, F["reads"].offs, F["regs"],
                                                  F["reg_off"], _aln_opt(F))
    cov = O.coverage(name, zip(F["regs"], want))
    print(f"host reg2aln {name}: {F['regs'].size} regions, kernel {ms:.3f} ms, {cov}")
    assert alns.size == F["regs"].size
    got = [T._got(alns, cigar, md, k) for k in range(alns.size)]
    n = 0
    for r, recs in enumerate(F["records"]):
        for w, h in zip(recs or [], F["hits"][r]):
            if h >= 0:
                a = got[h]
                assert (a.is_rev, a.pos, a.cigar, a.NM, a.md) == O.record_tuple(F, w), (r, w, a)
                n += 1
    assert n == F["man"]["matched"]
    bad = [(k, got[k], want[k]) for k in range(alns.size) if got[k] != want[k]]
    assert not bad, (len(bad), bad[:3])
    assert int(alns["n_cigar"].sum()) == cigar.size and int(alns["md_len"].sum()) == md.size


def _fin_records_equal(F, fin):
    """the reference's records of every read against smem_reg_finalize's output"""
    for r in range(F["lens"].size):
        want = F["records"][r]
        if want is None:
            continue
        lo, hi = int(fin.out_off[r]), int(fin.out_off[r + 1])
        idx = [int(k) - lo for k in fin.sel_idx[int(fin.sel_off[r]):int(fin.sel_off[r + 1])]]
        sel = [(int(s["mapq"]), int(s["flag"]), int(s["xs"])) for s in fin.sel[lo:hi]]
        got = D.predict_records(F, r, fin.regs[lo:hi], sel, idx)
        assert len(got) == len(want), (r, got, want)
        for g, w in zip(got, want):
            assert all(g[k] == w[k] for k in ("flag", "mapq", "AS", "XS")), (r, g, w)
            assert g["pos"] is None or (g["rname"], g["pos"]) == (w["rname"], w["pos"]), (r, g, w)


@pytest.mark.parametrize("name", O.SETS)
def test_host_reg_finalize(handles, name):
    """smem_reg_finalize under the set's options (T = 30 a, min_seed_len): every output
    field equals the restatement, every read's records equal the reference's"""
    F = O.load(name)
    fin = handles(F["g"]).reg_finalize(F["lens"], F["regs"], F["reg_off"], opt=_fin_opt(F), ids=F["ids"])
    print(f"host reg_finalize {name}: {F['regs'].size} -> {fin.regs.size} regions, {fin.sel_idx.size} records, "
          f"kernel {fin.kernel_ms:.3f} ms")
    D.assert_equal(fin, O.fin_arrays(name))
    _fin_records_equal(F, fin)


def _resident(gpu, F):
    """the whole chain on one batch; returns (fetched results, stats) of a reg2aln call
    made by `align(batch)` after reg_finalize"""
    import smemgpu
    reads, o = F["reads"], F["opt"]
    b = gpu.batch(reads.n, reads.codes.size, int(reads.lens.max()))
    b.set_reads(reads.codes, reads.offs)
    b.run(smemgpu.Options(min_seed_len=o["min_seed_len"]))
    b.sa(o["min_seed_len"], 10000)
    b.chain(F["l_pac"], w=o["w"])
    b.chain2aln(_aln_opt(F))
    b.reg_finalize(_fin_opt(F), ids=F["ids"])
    return b


def _records(aln):
    return [T._got(aln.alns, aln.cigar, aln.md, k) for k in range(aln.alns.size)]


def _check_resident(name, res, st):
    """records against the reference and the combined restatements, counters against the
    restated classifier; returns the coverage"""
    from smemgpu.lib import ALN_XREF
    F = O.load(name)
    names = [c[0] for c in F["contigs"]]
    offs = {c[0]: c[1] for c in F["contigs"]}
    _n, c_offs, c_lens = X.table(F["contigs"])
    fin, aln = res.fin, res.aln
    want = [t for row in O.expected(name) for t in row]
    got = _records(aln)
    assert np.array_equal(aln.aln_off, fin.sel_off) and aln.alns.size == fin.sel_idx.size == st["n_g2a"] == len(want)
    # the reference's records
    n = 0
    for r in range(F["lens"].size):
        lo, hi = int(fin.sel_off[r]), int(fin.sel_off[r + 1])
        recs = F["records"][r] or []
        assert hi - lo == len(recs), (r, hi - lo, recs)
        for k, w in zip(range(lo, hi), recs):
            a, s, p = got[k], fin.sel[int(fin.sel_idx[k])], fin.regs[int(fin.sel_idx[k])]
            assert int(s["mapq"]) == w["mapq"], (r, w)
            n += 1
            fix = X.needs_fix(c_offs, c_lens, F["l_pac"], int(p["rb"]), int(p["re"]))
            assert (a.status == ALN_XREF) == fix, (r, w, a)
            if fix:   # bwa_fix_xref2's: the mark and nothing else
                assert a.pos == -1 and a.cigar == () and int(aln.rid[k]) == -1
                assert int(s["flag"]) | (16 if int(p["rb"]) >= F["l_pac"] else 0) == w["flag"], (r, w)
                continue
            assert a.status == 0 and int(s["flag"]) | (16 if a.is_rev else 0) == w["flag"], (r, w)
            assert names[int(aln.rid[k])] == w["rname"], (r, w, int(aln.rid[k]))
            assert (a.pos - offs[w["rname"]] + 1, a.cigar, a.NM, a.md) == (w["pos"], w["ops"], w["nm"], w["md"]), (r, w, a)
    assert n == F["man"]["records"]
    # the restatements: every field, rid, the pools
    for k, (g, (p, w, rid)) in enumerate(zip(got, want)):
        assert g == w, (k, p, g, w)
        assert int(aln.rid[k]) == rid, (k, p, int(aln.rid[k]), rid)
    words, md_bytes = sum(len(w.cigar) for _p, w, _r in want), sum(len(w.md) for _p, w, _r in want)
    assert (int(aln.alns["n_cigar"].sum()), int(aln.alns["md_len"].sum())) == (aln.cigar.size, aln.md.size) == (words, md_bytes)
    # the counters
    cov = O.coverage(name, [(p, w) for p, w, _r in want])
    assert st["n_g2a_deferred"] == sum(cov["deferred"].values()), (st["n_g2a_deferred"], cov)
    assert st["n_g2a_xref"] == sum(1 for _p, w, _r in want if w.status == X.XREF)
    return cov, words, md_bytes


@pytest.mark.parametrize("name", O.SETS)
def test_resident_chain(handles, name):
    """run, sa, chain, chain2aln, reg_finalize, reg2aln under the set's options: the fetched
    raw regions are the committed ones byte for byte; every record equals the reference's
    and the restatements; n_g2a_deferred, n_g2a_xref and n_g2a_passes are what the
    restatements predict (two passes only past g2a_pool_estimate's 16 words / 48 bytes a
    record)"""
    from smemgpu.lib import FETCH_ALN, FETCH_FIN, FETCH_REGS
    F = O.load(name)
    b = _resident(handles(F["g"]), F)
    try:
        b.reg2aln(_aln_opt(F))
        res = b.fetch(FETCH_ALN | FETCH_FIN | FETCH_REGS)
        st = b.stats()
    finally:
        b.close()
    raw = np.frombuffer(res.regs.tobytes(), dtype=golden_data.ALNREG_DT)
    assert np.array_equal(res.reg_off, F["reg_off"]) and raw.tobytes() == F["regs"].tobytes()
    D.assert_equal(res.fin, O.fin_arrays(name))
    cov, words, md_bytes = _check_resident(name, res, st)
    n_rec = st["n_g2a"]
    print(f"resident {name}: records {n_rec}, deferred {st['n_g2a_deferred']}, xref {st['n_g2a_xref']}, "
          f"passes {st['n_g2a_passes']}, classes {cov['classes']}, tries {cov['tries']}, "
          f"{words} CIGAR words, {md_bytes} MD bytes, g2a {st['g2a_ms']:.3f} ms")
    assert st["n_g2a_passes"] == (2 if words > 16 * n_rec or md_bytes > 48 * n_rec else 1)


def test_resident_chain_deferrals_with_forced_pools(handles):
    """g1 r3 w7 (five deferrals, a multi-pass retry in the 16-lane kernel) with
    SMEM_G2A_POOL=1:1: the first pass overflows both pools, the second returns the records
    of the default run; deferral and pool regrowth in one call"""
    from smemgpu.lib import FETCH_ALN, FETCH_FIN
    name = "g1_r3_w7"
    F = O.load(name)
    b = _resident(handles(F["g"]), F)
    old = os.environ.get("SMEM_G2A_POOL")
    try:
        b.reg2aln(_aln_opt(F))
        want, st0 = b.fetch(FETCH_ALN).aln, b.stats()
        os.environ["SMEM_G2A_POOL"] = "1:1"
        b.reg2aln(_aln_opt(F))
        res, st1 = b.fetch(FETCH_ALN | FETCH_FIN), b.stats()
    finally:
        if old is None:
            os.environ.pop("SMEM_G2A_POOL", None)
        else:
            os.environ["SMEM_G2A_POOL"] = old
        b.close()
    assert (st0["n_g2a_passes"], st1["n_g2a_passes"]) == (1, 2)
    assert st0["n_g2a_deferred"] == st1["n_g2a_deferred"] == 5
    assert _records(res.aln) == _records(want) and np.array_equal(res.aln.rid, want.rid)
    _check_resident(name, res, st1)
