"""Raw regions -> final regions on the GPU (smem_reg_finalize,
smem_batch_reg_finalize): mem_sort_and_dedup, mem_test_and_remove_exact,
mem_mark_primary_se and the selection, MAPQ and flags of mem_reg2sam_se /
mem_reg2aln (software/bwamem.c:705-785, 1333-1379).

Bar: exact.  The GPU equals the Python restatement (tests/regfin_ref.py, pinned
to the reference's own SAM records by tests/test_regfin.py) in every field of
every output, and the reference's records directly on the five fixture sets.
mem_test_and_remove_exact after a de-duplication is reached by no command of
the committed reference harness: NO_EXACT is checked against the restatement
only.
"""
import os

import numpy as np
import pytest

import regfin_data as D
import regfin_ref as ref
from tests import golden_data

pytestmark = pytest.mark.gpu


def _c_opt(o: ref.Opt):
    import smemgpu
    return smemgpu.fin_opt(a=o.a, b=o.b, o_del=o.o_del, e_del=o.e_del, o_ins=o.o_ins, e_ins=o.e_ins,
                           min_seed_len=o.min_seed_len, T=o.T, mask_level=o.mask_level,
                           mask_level_redun=o.mask_level_redun, mapQ_coef_len=o.mapQ_coef_len,
                           mapQ_coef_fac=o.mapQ_coef_fac, no_exact=o.no_exact, all=o.all, no_multi=o.no_multi)


@pytest.fixture(scope="module")
def gpu(gpu_device):
    """one handle for the module; the stage needs no index, any small one opens the device"""
    import smemgpu
    from smemgpu import synth
    g = smemgpu.Gpu(smemgpu.Index.build(synth.make_genome(20_000, seed=3).codes), device=gpu_device)
    yield g
    g.close()


def _records_equal(F, fin, keys):
    """the reference's mapped records of every read against the stage's output"""
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
            assert all(g[k] == w[k] for k in keys), (r, g, w)
            assert g["pos"] is None or (g["rname"], g["pos"]) == (w["rname"], w["pos"]), (r, g, w)


@pytest.mark.parametrize("name", D.SETS)
def test_host_call_fixture_sets(gpu, name):
    """the host-buffer call over the reference's regions: every output field equals the
    restatement, every read's records equal the reference's"""
    F = D.load(name)
    fin = gpu.reg_finalize(F["lens"], F["regs"], F["reg_off"], ids=F["ids"])
    print(f"reg_finalize {name}: {F['regs'].size} -> {fin.regs.size} regions, {fin.sel_idx.size} records, "
          f"kernel {fin.kernel_ms:.3f} ms")
    D.assert_equal(fin, D.restate(ref.Opt(), F["regs"], F["reg_off"], F["lens"], F["ids"]))
    _records_equal(F, fin, ("flag", "mapq", "AS", "XS"))


def test_resident_stage_after_chain2aln(gpu_device, tmp_path):
    """g2_default_std through the real batch (seed, SA, chain, chain2aln), then the resident
    stage, fetched with SMEM_FETCH_FIN alone; SMEM_FETCH_REGS still returns the raw regions
    byte for byte, and they are the reference's"""
    import smemgpu
    from smemgpu.lib import FETCH_FIN, FETCH_REGS
    from oracle import oracle
    F = D.load("g2_default_std")
    fix = next(f for f in golden_data.aln_fixtures() if f["file"] == "g2_default_std.smrg.gz")
    reads = golden_data.aln_reads(fix)
    paths = golden_data.files("g2", str(tmp_path))
    gpu = smemgpu.Gpu(smemgpu.Index.read(paths["bwt"]), device=gpu_device)
    try:
        gpu.load_sa(smemgpu.SA.read(paths["sa"]))
        gpu.load_pac(golden_data.pac("g2"), F["l_pac"])
        b = gpu.batch(reads.n, reads.codes.size, int(reads.lens.max()))
        try:
            b.set_reads(reads.codes, reads.offs)
            b.run(smemgpu.Options())
            b.sa(19, 10000)
            b.chain(F["l_pac"])
            b.chain2aln(oracle.aln_opt())
            mem0 = b.memory()
            raw0 = b.fetch(FETCH_REGS)
            b.reg_finalize(ids=F["ids"])
            res = b.fetch(FETCH_FIN)
            assert res.regs is None and res.intv is None and res.chains is None
            raw1 = b.fetch(FETCH_REGS)
            assert raw1.fin is None
            st = b.stats()
            assert b.memory()[0] > mem0[0]      # the stage's buffers came with its first call
        finally:
            b.close()
    finally:
        gpu.close()
    fin = res.fin
    assert raw1.regs.tobytes() == raw0.regs.tobytes() and np.array_equal(raw1.reg_off, raw0.reg_off)
    raw = np.frombuffer(raw0.regs.tobytes(), dtype=golden_data.ALNREG_DT)
    assert np.array_equal(raw0.reg_off, F["reg_off"]) and raw.tobytes() == F["regs"].tobytes()
    assert (st["n_fin"], st["n_fin_sel"]) == (fin.regs.size, fin.sel_idx.size) and st["fin_ms"] > 0
    D.assert_equal(fin, D.restate(ref.Opt(), F["regs"], F["reg_off"], F["lens"], F["ids"]))
    _records_equal(F, fin, ("flag", "mapq", "AS", "XS"))


@pytest.mark.parametrize("g", ["g1", "g2"])
def test_chained_finalize_gather_reg2aln(gpu, g):
    """finalize, gather regs[sel_idx], then smem_reg2aln as it is: each record of the
    reference in flag, position, MAPQ, CIGAR, NM and MD (a region that bridges a contig boundary
    is bwa_fix_xref2's, the caller's: its flag and MAPQ only)"""
    import reg2aln_ref
    import test_reg2aln as T
    F = D.load("cigar_" + g)
    A = T._fixture(g)
    ctg = T._contigs(g)
    fin = gpu.reg_finalize(F["lens"], F["regs"], F["reg_off"], ids=F["ids"])
    alns, cigar, md, _ = gpu.reg2aln(A["pac"], A["l_pac"], A["reads"].codes, A["reads"].offs,
                                     fin.regs[fin.sel_idx.astype(np.int64)], fin.sel_off, T._c_opt(reg2aln_ref.Opt()))
    want_fin = D.restate(ref.Opt(), F["regs"], F["reg_off"], F["lens"], F["ids"])
    n = n_bridge = 0
    for r in range(F["lens"].size):
        lo, hi = int(fin.sel_off[r]), int(fin.sel_off[r + 1])
        assert hi - lo == len(F["records"][r])
        for k, w in zip(range(lo, hi), F["records"][r]):
            a = T._got(alns, cigar, md, k)
            s = fin.sel[int(fin.sel_idx[k])]
            p = fin.regs[int(fin.sel_idx[k])]
            assert int(s["mapq"]) == w["mapq"] == int(want_fin["sel"][int(fin.sel_idx[k])][0]), (r, w)
            n += 1
            if D.predict_records(F, r, [p], [(0, 0, 0)], [0])[0]["pos"] is None:
                assert int(s["flag"]) | (16 if int(p["rb"]) >= F["l_pac"] else 0) == w["flag"], (r, w)
                n_bridge += 1
                continue
            assert int(s["flag"]) | (16 if a.is_rev else 0) == w["flag"], (r, w)
            assert (a.pos, a.cigar, a.NM, a.md) == (ctg[w["rname"]] + w["pos"] - 1, T._sam_ops(w["cigar"]), w["nm"],
                                                     w["md"]), (r, w, a)
    assert n == (377 if g == "g1" else 379) and n_bridge <= 2


# ------------------------------------------------------------------ synthetic
OPTS = [dict(), dict(all=True), dict(no_multi=True, T=35), dict(no_exact=True),
        dict(mapQ_coef_len=0.0, mapQ_coef_fac=0), dict(mask_level=0.3, mask_level_redun=0.8, a=2, b=3, T=10)]


@pytest.fixture(scope="module")
def synth():
    """reads of every size at which the stage takes another path: 0-3, the lane / wave tier
    boundary 16 +- 1 (17, 18), 33-35, the wave passes 63-65 and 129, one that reaches the
    combsort, the limit 1024 and one past it"""
    rng = np.random.default_rng(5)
    big = [D.synth_regions(rng, 3), D.synth_regions(rng, ref.MAX_REGS, span=3000, qspan=100),
           D.synth_regions(rng, ref.MAX_REGS + 1), D.synth_regions(rng, 4)]
    regs, reg_off, lens = D.synth_reads(extra=big)
    regs["truesc"] = np.where(np.arange(regs.size) % 2 == 0, 100, regs["truesc"])   # = l_query * a: NO_EXACT bites
    return regs, reg_off, lens


@pytest.mark.parametrize("kw", OPTS, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()) or "default")
def test_synthetic_shapes_and_options(gpu, synth, kw):
    regs, reg_off, lens = synth
    opt = ref.Opt(**kw)
    ids = (1 << 33) + np.arange(lens.size, dtype=np.int64) * 3
    ctr = ref.Counters()
    want = D.restate(opt, regs, reg_off, lens, ids, ctr)
    fin = gpu.reg_finalize(lens, regs, reg_off, _c_opt(opt), ids=ids)
    D.assert_equal(fin, want)
    assert ctr.combsort > 0
    # the read past the limit is rejected, its neighbours are not
    k = int(np.nonzero(np.diff(reg_off.astype(np.int64)) > ref.MAX_REGS)[0][0])
    assert fin.status[k] == 1 and fin.out_off[k] == fin.out_off[k + 1] and fin.status.sum() == 1
    assert fin.out_off[k + 2] > fin.out_off[k + 1] and fin.out_off[k] > fin.out_off[k - 1]
    if kw.get("no_exact"):
        assert fin.regs.size < D.restate(ref.Opt(), regs, reg_off, lens, ids)["regs"].size
    if kw.get("all"):
        assert (fin.sel["flag"] == 0x100).any()
    if kw.get("no_multi"):
        assert (fin.sel["flag"] == 0x10000).any() and not (fin.sel["flag"] == 0x800).any()


def _reg(rb, re_, qb, qe, score, **kw):
    from smemgpu.lib import ALNREG_DT
    a = np.zeros(1, dtype=ALNREG_DT)
    a["rb"], a["re"], a["qb"], a["qe"], a["score"], a["truesc"], a["w"], a["seedcov"] = rb, re_, qb, qe, score, score, \
        100, qe - qb
    for k, v in kw.items():
        a[k] = v
    return a


def _reads(*reads):
    parts = [np.concatenate(r) for r in reads]
    reg_off = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)
    return np.concatenate(parts), reg_off, np.full(len(parts), 150, dtype=np.int32)


def test_float_overlaps_and_ids(gpu):
    """19 of 20 is not redundant at 0.95 and 10 of 20 is a significant overlap at 0.5 (both
    float products); id0 = 2^33 and explicit ids in paired-end form give the hashes"""
    regs, reg_off, lens = _reads(
        [_reg(100, 120, 0, 20, 30), _reg(101, 121, 1, 21, 31)],        # overlap 19 of 20: both stay
        [_reg(100, 120, 0, 20, 30), _reg(100, 121, 0, 21, 31)],        # 20 of 20: one goes
        [_reg(100, 120, 0, 20, 32), _reg(500, 520, 10, 30, 31)],       # query overlap 10 of 20: secondary
        [_reg(100, 120, 0, 20, 32), _reg(500, 520, 11, 31, 31)])       # 9 of 20: both primary
    fin = gpu.reg_finalize(lens, regs, reg_off, id0=1 << 33)
    assert np.diff(fin.out_off.astype(np.int64)).tolist() == [2, 1, 2, 2]
    assert fin.regs["score"][2] == 31                                   # the better of the redundant pair
    assert fin.regs["secondary"][3:].tolist() == [-1, 0, -1, -1]
    assert fin.regs["sub"][3] == 31 and fin.regs["sub_n"][3] == 1
    ids0 = (1 << 33) + np.arange(4, dtype=np.int64)
    D.assert_equal(fin, D.restate(ref.Opt(), regs, reg_off, lens, ids0))
    assert int(fin.regs["hash"][2]) == ref.hash_64((1 << 33) + 1)
    pe = (np.array([7, 7, 8, 8], dtype=np.int64) << 1) | np.array([0, 1, 0, 1])
    fin = gpu.reg_finalize(lens, regs, reg_off, ids=pe)
    D.assert_equal(fin, D.restate(ref.Opt(), regs, reg_off, lens, pe))
    assert sorted(int(h) for h in fin.regs["hash"][:2]) == sorted(ref.hash_64(14 + i) for i in range(2))


def test_mapq_cases(gpu):
    """MAPQ at l = 49 / 50 (the mapQ_coef_len switch), score 0, sub >= score, the cap at 60,
    the cap of a supplementary record at the first record's, a non-zero incoming sub_n, and
    arguments past the tables (-1: the caller computes it)"""
    reads = [
        [_reg(1000, 1049, 0, 49, 25)], [_reg(1000, 1050, 0, 50, 25)], [_reg(1000, 1049, 0, 49, 30, sub_n=3)],
        [_reg(1000, 1100, 0, 100, 0)],
        [_reg(1000, 1100, 0, 100, 60), _reg(9000, 9100, 0, 100, 60)],                  # sub >= score
        [_reg(1000, 1150, 0, 150, 150)],                                               # 60
        [_reg(1000, 1050, 0, 50, 50), _reg(9000, 9050, 0, 50, 48), _reg(5000, 5050, 50, 100, 45)],   # the cap
        [_reg(1000, 1000 + ref.TAB_LEN - 1, 0, 100, 90)], [_reg(1000, 1000 + ref.TAB_LEN, 0, 100, 90)],
        [_reg(1000, 1100, 0, 100, 90, sub_n=ref.TAB_LEN - 1)], [_reg(1000, 1100, 0, 100, 90, sub_n=ref.TAB_LEN)],
        [_reg(1000, 1000 + ref.TAB_LEN, 0, 50, 50), _reg(5000, 5050, 50, 100, 45)],    # -1 caps what follows
    ]
    regs, reg_off, lens = _reads(*reads)
    ids = np.arange(lens.size, dtype=np.int64)
    for kw in (dict(T=0), dict(T=0, mapQ_coef_len=0.0, mapQ_coef_fac=0)):
        opt = ref.Opt(**kw)
        fin = gpu.reg_finalize(lens, regs, reg_off, _c_opt(opt))
        D.assert_equal(fin, D.restate(opt, regs, reg_off, lens, ids))
        mq = [fin.sel["mapq"][int(fin.out_off[r]):int(fin.out_off[r + 1])].tolist() for r in range(lens.size)]
        if not kw.get("mapQ_coef_fac", 3) == 0:
            assert 0 < mq[1][0] < mq[0][0] < 60 and 0 < mq[2][0] < 60 and mq[3] == [0] and mq[4][0] == 0 and mq[5] == [60]
            assert mq[6][2] == mq[6][0] and mq[6][0] < 60        # capped at the first record's
            assert mq[7][0] >= 0 and mq[8] == [-1] and mq[9][0] >= 0 and mq[10] == [-1] and mq[11] == [-1, -1]
    # seedcov past its table, where the reference reads log(seedcov)
    regs2, off2, lens2 = _reads([_reg(1000, 1100, 0, 100, 90, seedcov=ref.TAB_LEN)],
                                [_reg(1000, 1100, 0, 100, 90, seedcov=ref.TAB_LEN - 1)])
    opt = ref.Opt(mapQ_coef_len=0.0, mapQ_coef_fac=0)
    fin = gpu.reg_finalize(lens2, regs2, off2, _c_opt(opt))
    D.assert_equal(fin, D.restate(opt, regs2, off2, lens2, np.arange(2)))
    assert fin.sel["mapq"].tolist()[0] == -1 and fin.sel["mapq"].tolist()[1] >= 0


def test_malformed_input_is_refused(gpu):
    import smemgpu
    regs, reg_off, lens = _reads([_reg(100, 120, 0, 20, 30)], [_reg(100, 120, 0, 20, 30)])
    bad = regs.copy()
    bad["qe"][1] = bad["qb"][1] - 1
    with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
        gpu.reg_finalize(lens, bad, reg_off)
    with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
        gpu.reg_finalize(lens, np.concatenate([regs, regs]), np.array([0, 3, 2], dtype=np.uint64))
    assert gpu.fault()[0] == 0
    fin = gpu.reg_finalize(lens, regs, reg_off)
    assert fin.regs.size == 2


def test_injected_failure_keeps_earlier_results(gpu_device):
    """SMEM_GPU_FAIL=fin:1: the stage returns SMEM_E_DEVICE, the device is not faulted, the
    batch's earlier results stay fetchable and the stage then runs"""
    import smemgpu
    from smemgpu import synth
    from smemgpu.lib import FETCH_FIN, FETCH_REGS
    from oracle import oracle
    g = synth.make_genome(60_000, seed=21, repeat_frac=0.4, n_families=3)
    idx, sa = smemgpu.Index.build_sa(g.codes)
    reads = synth.make_reads(g.codes, 300, 120, seed=22, sub_rate=0.02)
    c = np.concatenate([g.codes, np.zeros((-g.codes.size) % 4, np.uint8)]).reshape(-1, 4).astype(np.uint8)
    pac = (c[:, 0] << 6 | c[:, 1] << 4 | c[:, 2] << 2 | c[:, 3]).astype(np.uint8)
    gpu = smemgpu.Gpu(idx, device=gpu_device)
    old = os.environ.get("SMEM_GPU_FAIL")
    try:
        gpu.load_sa(sa)
        gpu.load_pac(pac, int(g.codes.size))
        b = gpu.batch(reads.n, reads.codes.size, int(reads.lens.max()))
        b.set_reads(reads.codes, reads.offs)
        b.run(smemgpu.Options())
        b.sa(19, 10000)
        b.chain(int(g.codes.size))
        b.chain2aln(oracle.aln_opt())
        raw0 = b.fetch(FETCH_REGS)
        os.environ["SMEM_GPU_FAIL"] = "fin:1"
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_DEVICE.*injected"):
            b.reg_finalize()
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_DEVICE.*injected"):
            gpu.reg_finalize(reads.lens, raw0.regs, raw0.reg_off)
        os.environ.pop("SMEM_GPU_FAIL")
        assert gpu.fault()[0] == 0
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
            b.fetch(FETCH_FIN)                      # the stage has not run
        raw1 = b.fetch(FETCH_REGS)
        assert raw1.regs.tobytes() == raw0.regs.tobytes() and raw0.regs.size > 0
        b.reg_finalize()
        fin = b.fetch(FETCH_FIN).fin
        b.close()
    finally:
        if old is None:
            os.environ.pop("SMEM_GPU_FAIL", None)
        else:
            os.environ["SMEM_GPU_FAIL"] = old
        gpu.close()
    regs = np.frombuffer(raw0.regs.tobytes(), dtype=golden_data.ALNREG_DT)
    D.assert_equal(fin, D.restate(ref.Opt(), regs, raw0.reg_off, reads.lens, np.arange(reads.n)))
