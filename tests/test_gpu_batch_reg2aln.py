"""Final regions -> alignments as a device-resident batch stage
(smem_batch_reg2aln, Batch.reg2aln) with the contig lookup
(smem_gpu_load_contigs): seeding, SA, chaining, chains -> regions, finalize and
the alignment of every record without a region crossing to the host.

Bar: exact.  Every record equals the restatements (tests/regfin_ref.py,
tests/reg2aln_ref.py, tests/xref_ref.py, each pinned to the reference's own
records without a GPU) in every field, the reference's records directly in
flag, contig, position, MAPQ, CIGAR, NM and MD, and the host-buffer call
(smem_reg2aln) over the same gathered regions.  A region that bridges a contig
boundary is bwa_fix_xref2's: it must carry SMEM_ALN_XREF and nothing else.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import reg2aln_ref
import regfin_data as D
import test_reg2aln as T
import xref_ref as X
from tests import golden_data

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def handles(gpu_device, tmp_path_factory):
    """one handle per (genome, with / without a contig table), opened on first use: index,
    .sa and .pac resident"""
    import smemgpu
    made = {}

    def get(g, contigs=True):
        if (g, contigs) not in made:
            paths = golden_data.files(g, str(tmp_path_factory.mktemp(g)))
            gpu = smemgpu.Gpu(smemgpu.Index.read(paths["bwt"]), device=gpu_device)
            gpu.load_sa(smemgpu.SA.read(paths["sa"]))
            gpu.load_pac(golden_data.pac(g), golden_data.l_pac(g))
            if contigs:
                _n, offs, lens = X.table(D.contigs(g))
                gpu.load_contigs(offs, lens, golden_data.l_pac(g))
            made[(g, contigs)] = gpu
        return made[(g, contigs)]
    yield get
    for gpu in made.values():
        gpu.close()


def _to_finalize(gpu, name):
    """a batch over the set's reads, run up to reg_finalize"""
    import smemgpu
    from oracle import oracle
    F = D.load(name)
    reads = X.reads_of(name)
    b = gpu.batch(reads.n, reads.codes.size, int(reads.lens.max()))
    b.set_reads(reads.codes, reads.offs)
    b.run(smemgpu.Options())
    b.sa(19, 10000)
    b.chain(F["l_pac"])
    b.chain2aln(oracle.aln_opt())
    b.reg_finalize(ids=F["ids"])
    return b


def _opt():
    return T._c_opt(reg2aln_ref.Opt())


def _records(aln):
    return [T._got(aln.alns, aln.cigar, aln.md, k) for k in range(aln.alns.size)]


def _check_against_restatement(name, res, contigs=True):
    """every smem_aln_t field and rid of every record; returns the records flattened"""
    want = [t for row in X.expected(name, contigs) for t in row]
    got = _records(res.aln)
    assert len(got) == len(want) == res.aln.rid.size
    for k, (g, (p, w, rid)) in enumerate(zip(got, want)):
        assert g == w, (k, p, g, w)
        assert int(res.aln.rid[k]) == rid, (k, p, int(res.aln.rid[k]), rid)
    used = int(res.aln.alns["n_cigar"].sum()), int(res.aln.alns["md_len"].sum())
    assert used == (res.aln.cigar.size, res.aln.md.size)
    return got, want


@pytest.mark.parametrize("g", ["g1", "g2"])
def test_resident_chain_gapped_reads(handles, g):
    """the gapped reads of tests/golden/cigar/: raw regions are the reference's, then every
    record of the reference in flag, contig, position, MAPQ, CIGAR, NM and MD"""
    from smemgpu.lib import ALN_XREF, FETCH_ALN, FETCH_FIN, FETCH_REGS
    name = "cigar_" + g
    F = D.load(name)
    names = [c[0] for c in F["contigs"]]
    offs = {c[0]: c[1] for c in F["contigs"]}
    b = _to_finalize(handles(g), name)
    try:
        b.reg2aln(_opt())
        res = b.fetch(FETCH_ALN | FETCH_FIN | FETCH_REGS)
        st = b.stats()
    finally:
        b.close()
    print(f"batch reg2aln {name}: {st['n_g2a']} records, {st['n_g2a_deferred']} deferred, {st['n_g2a_xref']} xref, "
          f"g2a {st['g2a_ms']:.3f} ms (prep {st['g2a_prep_ms']:.3f} ms), passes {st['n_g2a_passes']}")
    raw = np.frombuffer(res.regs.tobytes(), dtype=golden_data.ALNREG_DT)
    assert np.array_equal(res.reg_off, F["reg_off"]) and raw.tobytes() == F["regs"].tobytes()
    fin, aln = res.fin, res.aln
    assert np.array_equal(aln.aln_off, fin.sel_off) and aln.alns.size == fin.sel_idx.size == st["n_g2a"]
    assert st["n_g2a_passes"] == 1 and st["g2a_ms"] > 0 and st["g2a_ms"] >= st["g2a_prep_ms"] > 0
    got, _want = _check_against_restatement(name, res)
    n = n_bridge = 0
    for r in range(F["lens"].size):
        lo, hi = int(fin.sel_off[r]), int(fin.sel_off[r + 1])
        assert hi - lo == len(F["records"][r])
        for k, w in zip(range(lo, hi), F["records"][r]):
            a, s, p = got[k], fin.sel[int(fin.sel_idx[k])], fin.regs[int(fin.sel_idx[k])]
            assert int(s["mapq"]) == w["mapq"], (r, w)
            n += 1
            if a.status == ALN_XREF:
                assert D.predict_records(F, r, [p], [(0, 0, 0)], [0])[0]["pos"] is None, (r, w)   # only such regions
                assert a.pos == -1 and a.cigar == () and int(aln.rid[k]) == -1
                assert int(s["flag"]) | (16 if int(p["rb"]) >= F["l_pac"] else 0) == w["flag"], (r, w)
                n_bridge += 1
                continue
            assert a.status == 0 and int(s["flag"]) | (16 if a.is_rev else 0) == w["flag"], (r, w)
            assert names[int(aln.rid[k])] == w["rname"], (r, w, int(aln.rid[k]))
            assert (a.pos - offs[w["rname"]] + 1, a.cigar, a.NM, a.md) == (w["pos"], T._sam_ops(w["cigar"]), w["nm"],
                                                                             w["md"]), (r, w, a)
    assert n == (377 if g == "g1" else 379) and n_bridge <= 2 and n_bridge == st["n_g2a_xref"]


@pytest.mark.parametrize("g", ["g1", "g2"])
def test_resident_chain_default_reads(handles, g):
    """the golden single-end reads: SMEM_ALN_XREF exactly where the CPU test found it (at least
    once per genome), contig and position of every other record are the golden record's"""
    from smemgpu.lib import ALN_XREF, FETCH_ALN, FETCH_FIN
    name = g + "_default_std"
    F = D.load(name)
    names = [c[0] for c in F["contigs"]]
    offs = {c[0]: c[1] for c in F["contigs"]}
    b = _to_finalize(handles(g), name)
    try:
        b.reg2aln(_opt())
        res = b.fetch(FETCH_ALN | FETCH_FIN)
        st = b.stats()
    finally:
        b.close()
    assert np.array_equal(res.aln.aln_off, res.fin.sel_off)
    got, want = _check_against_restatement(name, res)
    xref = [k for k, a in enumerate(got) if a.status == ALN_XREF]
    assert xref == [k for k, (_p, w, _rid) in enumerate(want) if w.status == X.XREF] and 1 <= len(xref) <= 2
    assert st["n_g2a_xref"] == len(xref)
    for r, recs in enumerate(F["records"]):
        if recs is None:
            continue
        lo, hi = int(res.fin.sel_off[r]), int(res.fin.sel_off[r + 1])
        assert hi - lo == len(recs)
        for k, w in zip(range(lo, hi), recs):
            if got[k].status != ALN_XREF:
                assert names[int(res.aln.rid[k])] == w["rname"] and got[k].pos - offs[w["rname"]] + 1 == w["pos"], (r, w)


def _gathered_host_call(gpu, name, fin, idx, idx_off):
    """Gpu.reg2aln (the host-buffer call) over the final regions gathered by idx"""
    F, reads = D.load(name), X.reads_of(name)
    alns, cigar, md, _ = gpu.reg2aln(None, F["l_pac"], reads.codes, reads.offs, fin.regs[idx.astype(np.int64)], idx_off,
                                     _opt())
    return [T._got(alns, cigar, md, k) for k in range(alns.size)]


def test_without_contigs_equals_the_host_call(handles):
    """no table: rid -1 everywhere, nothing marked, every record what smem_reg2aln returns for
    the gathered regions (CIGAR words and MD bytes per record; the offsets may differ)"""
    from smemgpu.lib import ALN_XREF, FETCH_ALN, FETCH_FIN
    name = "cigar_g2"
    gpu = handles("g2", contigs=False)
    b = _to_finalize(gpu, name)
    try:
        b.reg2aln(_opt())
        res = b.fetch(FETCH_ALN | FETCH_FIN)
        st = b.stats()
    finally:
        b.close()
    assert (res.aln.rid == -1).all() and not (res.aln.alns["status"] == ALN_XREF).any() and st["n_g2a_xref"] == 0
    assert _records(res.aln) == _gathered_host_call(gpu, name, res.fin, res.fin.sel_idx, res.fin.sel_off)
    _check_against_restatement(name, res, contigs=False)


def test_callers_selection(handles):
    """idx / idx_off: all final regions (secondaries too), a reversed order, a duplicate, empty
    lists; each equals the host-buffer call over the same gathered regions; an index outside
    its read's range is refused"""
    import smemgpu
    from smemgpu.lib import FETCH_ALN, FETCH_FIN
    name = "cigar_g2"
    gpu = handles("g2", contigs=False)
    b = _to_finalize(gpu, name)
    try:
        fin = b.fetch(FETCH_FIN).fin
        n = fin.out_off.size - 1
        everything = np.arange(fin.regs.size, dtype=np.uint64)
        assert everything.size > fin.sel_idx.size          # more shapes than the selection has
        rev = np.concatenate([everything[int(fin.out_off[r]):int(fin.out_off[r + 1])][::-1] for r in range(n)])
        r2 = int(np.nonzero(np.diff(fin.out_off.astype(np.int64)) >= 2)[0][0])
        lo = int(fin.out_off[r2])
        dup = np.concatenate([everything[:lo + 1], [lo], everything[lo + 1:]]).astype(np.uint64)
        dup_off = fin.out_off.copy()
        dup_off[r2 + 1:] += 1
        cases = [("all", everything, fin.out_off), ("reversed", rev.astype(np.uint64), fin.out_off),
                 ("duplicate", dup, dup_off), ("empty", np.zeros(0, np.uint64), np.zeros(n + 1, np.uint64))]
        for what, idx, idx_off in cases:
            b.reg2aln(_opt(), idx, idx_off)
            res = b.fetch(FETCH_ALN)
            assert np.array_equal(res.aln.aln_off, idx_off) and res.aln.alns.size == idx.size, what
            assert (res.aln.rid == -1).all()
            if idx.size:
                assert _records(res.aln) == _gathered_host_call(gpu, name, fin, idx, idx_off), what
            else:
                assert res.aln.cigar.size == 0 and res.aln.md.size == 0 and b.stats()["n_g2a"] == 0
        # a region of the next read, and an index past the final regions
        bad = everything.copy()
        assert fin.out_off[r2 + 1] < fin.regs.size
        bad[int(fin.out_off[r2 + 1]) - 1] = fin.out_off[r2 + 1]
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
            b.reg2aln(_opt(), bad, fin.out_off)
        bad[-1] = fin.regs.size
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
            b.reg2aln(_opt(), bad, fin.out_off)
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
            b.fetch(FETCH_ALN)                              # a refused call leaves no results
        assert gpu.fault()[0] == 0
        b.reg2aln(_opt())                                   # and the batch goes on
        assert np.array_equal(b.fetch(FETCH_ALN).aln.aln_off, fin.sel_off)
    finally:
        b.close()


def test_pools_grow_in_a_second_pass(handles):
    """SMEM_G2A_POOL=1:1 (one word, one byte a record) cannot hold the output: the stage sizes
    the pools from the cursors, runs again and returns what the default run returns"""
    from smemgpu.lib import FETCH_ALN
    name = "cigar_g2"
    gpu = handles("g2")
    b = _to_finalize(gpu, name)
    old = os.environ.get("SMEM_G2A_POOL")
    try:
        b.reg2aln(_opt())
        want, st0 = b.fetch(FETCH_ALN).aln, b.stats()
        os.environ["SMEM_G2A_POOL"] = "1:1"
        b.reg2aln(_opt())
        res, st1 = b.fetch(FETCH_ALN), b.stats()
    finally:
        if old is None:
            os.environ.pop("SMEM_G2A_POOL", None)
        else:
            os.environ["SMEM_G2A_POOL"] = old
        b.close()
    assert (st0["n_g2a_passes"], st1["n_g2a_passes"]) == (1, 2) and st1["g2a_ms"] > st1["g2a_prep_ms"] > 0
    assert _records(res.aln) == _records(want) and np.array_equal(res.aln.rid, want.rid)
    assert int(res.aln.alns["n_cigar"].sum()) == res.aln.cigar.size > res.aln.alns.size
    assert int(res.aln.alns["md_len"].sum()) == res.aln.md.size > res.aln.alns.size
    _check_against_restatement(name, res)


def test_order_and_contract(handles, gpu_device):
    import smemgpu
    from oracle import oracle
    from smemgpu import synth
    from smemgpu.lib import FETCH_ALN, FETCH_FIN
    name = "cigar_g2"
    F = D.load(name)
    gpu = handles("g2")
    reads = X.reads_of(name)
    b = gpu.batch(reads.n, reads.codes.size, int(reads.lens.max()))
    try:
        b.set_reads(reads.codes, reads.offs)
        b.run(smemgpu.Options())
        b.sa(19, 10000)
        b.chain(F["l_pac"])
        b.chain2aln(oracle.aln_opt())
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
            b.reg2aln(_opt())                               # before reg_finalize
        b.reg_finalize(ids=F["ids"])
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
            b.fetch(FETCH_ALN)                              # before the stage
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
            b.reg2aln(T._c_opt(reg2aln_ref.Opt(e_del=0)))   # aln_opt_ok
        mem0 = b.memory()
        b.reg2aln(_opt())
        mem1 = b.memory()
        first = b.fetch(FETCH_ALN | FETCH_FIN)
        mem2 = b.memory()
        b.reg2aln(_opt())
        assert mem1[0] > mem0[0] and b.memory()[0] == mem2[0] == mem1[0]    # the stage's buffers: first call only
        again = b.fetch(FETCH_ALN)
        assert _records(again.aln) == _records(first.aln)
        b.chain2aln(oracle.aln_opt())                       # a later chain2aln ends the results
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
            b.fetch(FETCH_ALN)
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
            b.reg2aln(_opt())
        b.reg_finalize(ids=F["ids"])
        b.reg2aln(_opt())
        b.reg_finalize(ids=F["ids"])                        # and so does a later reg_finalize
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
            b.fetch(FETCH_ALN)
        # reads of N only: no regions, no records
        nn = synth.Reads(np.full(8, 100, np.int32), np.full(800, 4, np.uint8), np.arange(9, dtype=np.int64) * 100)
        b.set_reads(nn.codes, nn.offs)
        b.run(smemgpu.Options())
        b.sa(19, 10000)
        b.chain(F["l_pac"])
        b.chain2aln(oracle.aln_opt())
        b.reg_finalize()
        b.reg2aln(_opt())
        res = b.fetch(FETCH_ALN | FETCH_FIN)
        assert res.fin.regs.size == 0 and res.aln.alns.size == 0 and res.aln.rid.size == 0
        assert res.aln.cigar.size == 0 and res.aln.md.size == 0 and not res.aln.aln_off.any() and res.aln.aln_off.size == 9
    finally:
        b.close()
    # a table that does not tile [0, l_pac)
    _n, offs, lens = X.table(F["contigs"])
    assert offs.size >= 2
    gap = offs.copy()
    gap[1] += 1
    for o, l, lp in ((gap, lens, F["l_pac"]), (offs, lens, F["l_pac"] + 1), (offs[1:], lens[1:], F["l_pac"]),
                     (offs[:0], lens[:0], F["l_pac"])):
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
            gpu.load_contigs(o, l, lp)
    gpu.load_contigs(offs, lens, F["l_pac"])                # (loading again replaces the table)
    # no resident .pac: the stage cannot be reached past its argument checks
    g0 = smemgpu.Gpu(smemgpu.Index.build(synth.make_genome(20_000, seed=3).codes), device=gpu_device)
    try:
        b0 = g0.batch(4, 400, 100)
        b0.set_reads(nn.codes[:400], nn.offs[:5])
        b0.run(smemgpu.Options())
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
            b0.reg2aln(_opt())
        b0.close()
    finally:
        g0.close()


def test_reserved_slot_carries_the_stage(handles):
    """once the stage has run on a handle, smem_gpu_reserve_slots sizes a worker slot for it: the
    stage then runs on the slot's batch (smem_gpu_collect_ex) without growing it, same records"""
    import ctypes as C
    import smemgpu
    from oracle import oracle
    from smemgpu.lib import FETCH_ALN, FETCH_FIN, ChainOptT, COLLECT_NO_FETCH
    from test_gpu_product import _collect
    name, n = "cigar_g2", 64
    F, reads = D.load(name), X.reads_of(name)
    gpu = handles("g2")
    b = _to_finalize(gpu, name)
    try:
        b.reg2aln(_opt())                                   # the handle has seen the stage
    finally:
        b.close()
    lib = smemgpu.load()
    gpu.reserve_slots(1, n, int(reads.lens.max()))
    rc, bh, _keep = _collect(lib, gpu._h, 0, reads, 0, n, flags=COLLECT_NO_FETCH)   # (waits for its slot)
    assert rc == 0
    assert lib.smem_batch_sa(bh, 19, 10000) == 0
    co = ChainOptT(100, 10000, 0.5, 0.5, 1)
    assert lib.smem_batch_chain(bh, F["l_pac"], C.byref(co)) == 0
    ao, fo, o = oracle.aln_opt(), smemgpu.fin_opt(), _opt()
    assert lib.smem_batch_chain2aln(bh, C.byref(ao)) == 0
    ids = np.ascontiguousarray(F["ids"][:n], dtype=np.int64)
    assert lib.smem_batch_reg_finalize(bh, ids.ctypes.data, 0, C.byref(fo)) == 0
    d0, d1 = C.c_uint64(), C.c_uint64()
    assert lib.smem_batch_memory(bh, C.byref(d0), None) == 0
    assert lib.smem_batch_reg2aln(bh, C.byref(o), None, None) == 0
    assert lib.smem_batch_memory(bh, C.byref(d1), None) == 0
    assert d1.value == d0.value                             # the stage's buffers came with the slot
    assert lib.smem_batch_fetch_mask(bh, FETCH_ALN | FETCH_FIN) == 0
    al, cg, md = C.c_void_p(), C.POINTER(C.c_uint32)(), C.c_void_p()
    ri, nal, ncw, nmb = C.POINTER(C.c_int32)(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert lib.smem_batch_aln2_results(bh, C.byref(al), C.byref(ri), None, C.byref(cg), C.byref(ncw), C.byref(md),
                                       C.byref(nmb), C.byref(nal)) == 0
    k = int(nal.value)
    alns = np.frombuffer((C.c_char * (k * smemgpu.lib.ALN_DT.itemsize)).from_address(al.value), dtype=smemgpu.lib.ALN_DT)
    cigar = np.ctypeslib.as_array(cg, shape=(int(ncw.value),))
    mdb = np.frombuffer((C.c_char * int(nmb.value)).from_address(md.value), dtype=np.uint8)
    want = [t for row in X.expected(name)[:n] for t in row]
    assert k == len(want) > 0
    for j, (_p, w, rid) in enumerate(want):
        assert T._got(alns, cigar, mdb, j) == w and int(ri[j]) == rid, (j, w)


_CHILD = r"""
import os, sys
import numpy as np
import smemgpu
from smemgpu import synth
from smemgpu.lib import FETCH_ALN, FETCH_FIN
from oracle import oracle
import reg2aln_ref, test_reg2aln as T

g = synth.make_genome(60_000, seed=21, repeat_frac=0.4, n_families=3)
idx, sa = smemgpu.Index.build_sa(g.codes)
reads = synth.make_reads(g.codes, 40, 120, seed=22, sub_rate=0.02)
pac, L = T._pack(g.codes), int(g.codes.size)
gpu = smemgpu.Gpu(idx, device=int(sys.argv[1]))
gpu.load_sa(sa)
gpu.load_pac(pac, L)
b = gpu.batch(reads.n, reads.codes.size, int(reads.lens.max()))
b.set_reads(reads.codes, reads.offs)
b.run(smemgpu.Options())
b.sa(19, 10000)
b.chain(L)
b.chain2aln(oracle.aln_opt())
b.reg_finalize()
fin0 = b.fetch(FETCH_FIN).fin
opt = T._c_opt(reg2aln_ref.Opt())
os.environ["SMEM_GPU_FAIL"] = sys.argv[2]
try:
    b.reg2aln(opt)
    raise SystemExit("the injected failure did not surface")
except smemgpu.SmemError as e:
    assert "SMEM_E_DEVICE" in str(e) and "injected" in str(e), e
os.environ.pop("SMEM_GPU_FAIL")
assert gpu.fault()[0] == 0
try:
    b.fetch(FETCH_ALN)
    raise SystemExit("results of a failed call were fetchable")
except smemgpu.SmemError as e:
    assert "SMEM_E_ARG" in str(e), e
fin1 = b.fetch(FETCH_FIN).fin                     # the earlier stage's results stay
assert fin1.regs.tobytes() == fin0.regs.tobytes() and np.array_equal(fin1.sel_idx, fin0.sel_idx) and fin0.sel_idx.size
b.reg2aln(opt)
res = b.fetch(FETCH_ALN).aln
b.close()
gpu.close()
assert np.array_equal(res.aln_off, fin0.sel_off)
rd = np.repeat(np.arange(reads.n), np.diff(fin0.sel_off.astype(np.int64)))
for k in range(res.alns.size):
    want = reg2aln_ref.reg2aln(reg2aln_ref.Opt(), L, pac, reads.read(int(rd[k])), fin0.regs[int(fin0.sel_idx[k])])
    assert T._got(res.alns, res.cigar, res.md, k) == want, (k, want)
print("child ok", res.alns.size)
"""


def test_injected_failure_in_a_child(gpu_device, built):
    """SMEM_GPU_FAIL=g2a:1 (the library's own return-code hook, after the work is enqueued): the
    call returns SMEM_E_DEVICE, the finalize results stay fetchable, the next call succeeds and
    equals the restatement"""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "bwa-mem-harp2_amd"), ROOT,
                                                       os.path.join(ROOT, "tests")]))
    env.pop("SMEM_GPU_FAIL", None)
    p = subprocess.run([sys.executable, "-c", _CHILD, str(gpu_device), "g2a:1"], capture_output=True, timeout=120,
                       env=env)
    out = p.stdout.decode(errors="replace") + p.stderr.decode(errors="replace")
    assert p.returncode == 0 and "child ok" in out, out[-3000:]
