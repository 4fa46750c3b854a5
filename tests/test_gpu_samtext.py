"""Alignments -> single-end SAM text on the GPU (smem_batch_sam after smem_batch_reg2aln,
smem_sam_text over host buffers; csrc/sam_kernels.hip).

Bar: exact.  The resident chain (seeding, SA, chaining, chains -> regions, finalize, reg2aln,
sam) gives the reference's own lines byte for byte for every read it does not leave to the host
(tests/golden/samtext/, sam/g1_se.sam.gz), and leaves exactly the reads the restatement lists
(tests/samtext_data.HOST_READS, at most 1 % of a set).  The host-buffer call equals the
restatement (tests/samtext_ref.py, pinned to the reference in tests/test_samtext.py) on
synthetic records at the smallest shapes at which the kernels can go wrong.  RG:Z, comments,
0x100 and 0x10000 records rest on the restatement's reading (tests/test_samtext.py).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import samtext_data as SD
import samtext_ref as S
import test_reg2aln as T
import reg2aln_ref
import xref_ref as X
from tests import golden_data

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def handles(gpu_device, tmp_path_factory):
    """one handle per genome, opened on first use: index, .sa, .pac, contig table and names resident"""
    import smemgpu
    made = {}

    def get(g):
        if g not in made:
            import regfin_data as D
            paths = golden_data.files(g, str(tmp_path_factory.mktemp(g)))
            gpu = smemgpu.Gpu(smemgpu.Index.read(paths["bwt"]), device=gpu_device)
            gpu.load_sa(smemgpu.SA.read(paths["sa"]))
            gpu.load_pac(golden_data.pac(g), golden_data.l_pac(g))
            names, offs, lens = X.table(D.contigs(g))
            gpu.load_contigs(offs, lens, golden_data.l_pac(g))
            gpu.load_contig_names(names)
            made[g] = gpu
        return made[g]
    yield get
    for gpu in made.values():
        gpu.close()


def _opt():
    return T._c_opt(reg2aln_ref.Opt())


def _to_reg2aln(gpu, F, text=True, finalize=True):
    import smemgpu
    from oracle import oracle
    reads = F["reads"]
    b = gpu.batch(reads.n, reads.codes.size, int(reads.lens.max()))
    b.set_reads(reads.codes, reads.offs)
    if text:
        b.set_read_text(F["names"], F["quals"])
    b.run(smemgpu.Options())
    b.sa(19, 10000)
    b.chain(F["l_pac"])
    b.chain2aln(oracle.aln_opt())
    if finalize:
        b.reg_finalize(ids=F["ids"])
        b.reg2aln(_opt())
    return b


@pytest.mark.parametrize("name", ["g1_r3_default", "g2_r4_default", "g1_default_std"])
def test_resident_chain(handles, name):
    from smemgpu.lib import FETCH_SAM, SAM_HOST
    F, want = SD.load(name), SD.texts(name)
    b = _to_reg2aln(handles(F["g"]), F)
    try:
        b.sam()
        sam = b.fetch(FETCH_SAM).sam
        st = b.stats()
    finally:
        b.close()
    print(f"batch sam {name}: {st['n_sam_bytes']} B, {st['n_sam_host']} reads to the host, sam {st['sam_ms']:.3f} ms "
          f"(write {st['sam_write_ms']:.3f} ms)")
    n = len(want)
    assert sam.text_off.size == n + 1 and sam.text_off[0] == 0 and (np.diff(sam.text_off.astype(np.int64)) >= 0).all()
    assert st["n_sam_bytes"] == sam.text.size == int(sam.text_off[-1]) and st["sam_ms"] > 0
    host = [r for r in range(n) if sam.status[r] == SAM_HOST]
    assert host == [r for r in range(n) if want[r] is None] and set(np.unique(sam.status)) <= {0, SAM_HOST}
    assert len(host) <= SD.HOST_CAP * n and st["n_sam_host"] == len(host)
    if name in SD.HOST_READS:
        assert host == SD.HOST_READS[name]
    n_golden = 0
    for r in range(n):
        got = sam.read(r)
        if r in host:
            assert got == b""
            continue
        assert got == want[r], (name, r, got, want[r])
        if F["golden"][r] is not None:
            assert got == F["golden"][r], (name, r)
            n_golden += 1
    assert n_golden >= 0.99 * sum(g is not None for g in F["golden"])
    # a batch's text can be written to a file as it is
    assert sam.text.tobytes() == b"".join(t for t in want if t is not None)


# ------------------------------------------------------------------ synthetic records
CTG_NAMES = ["c", "chr2_long_name.v1", "chrX", "chrBeyond4G", "k" * 40]
CTG_OFFS = [0, 1000, 1000 + (1 << 31) + 1000, (1 << 32) + 123_456_789, (1 << 33) + 7]
LENGTHS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 1024)


def _cigar(rng, L, n_words, clip5, clip3):
    """n_words words whose query span is L: clips at the ends, M / I / D in between (the first
    and last inner words M)"""
    inner_q = L - clip5 - clip3
    n_in = n_words - (clip5 > 0) - (clip3 > 0)
    assert n_in >= 1 and inner_q >= 1
    ops = [0 if i % 2 == 0 or i == n_in - 1 else (1, 2)[int(rng.integers(0, 2))] for i in range(n_in)]
    lens = [int(rng.integers(1, 120)) if o == 2 else 1 for o in ops]
    nq = sum(1 for o in ops if o != 2)
    assert nq <= inner_q, (L, n_words)
    lens[int(rng.integers(0, (n_in + 1) // 2)) * 2 if n_in > 1 else 0] += inner_q - nq   # the rest on one M
    words = [l << 4 | o for l, o in zip(lens, ops)]
    if clip5:
        words.insert(0, clip5 << 4 | 3)
    if clip3:
        words.append(clip3 << 4 | 3)
    assert sum(w >> 4 for w in words if (w & 0xf) != 2) == L and len(words) == n_words
    return tuple(words)


def _rec(rng, L, which, **kw):
    clip5 = int(rng.integers(1, max(2, L // 3))) if L >= 8 and rng.random() < 0.7 else 0
    clip3 = int(rng.integers(1, max(2, L // 3))) if L >= 8 and rng.random() < 0.7 else 0
    clip5, clip3 = kw.pop("clip5", clip5), kw.pop("clip3", clip3)
    n_words = kw.pop("n_words", None)
    if n_words is None:
        n_words = (clip5 > 0) + (clip3 > 0) + int(rng.integers(1, max(2, min(9, (L - clip5 - clip3 + 1) // 2))))
    rid = int(kw.pop("rid", rng.integers(0, len(CTG_NAMES))))
    pos1 = int(kw.pop("pos1", rng.integers(1, 900)))
    md = kw.pop("md", None)
    if md is None:
        md = "".join("ACGT^0123456789"[int(c)] for c in rng.integers(0, 15, int(rng.integers(1, 30))))
    r = S.Rec(rid=rid, pos=CTG_OFFS[rid] + pos1 - 1, is_rev=int(rng.integers(0, 2)),
              cigar=_cigar(rng, L, n_words, clip5, clip3), NM=int(rng.integers(0, 12)), md=md,
              mapq=int(rng.integers(0, 61)), flag=0x800 if which else 0, score=int(rng.integers(30, 1200)),
              xs=int(rng.integers(0, 300)))
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _read(rng, i, L, recs, name=None, fin_status=0):
    name = name if name is not None else "q" * (i % 40 + 1)
    return dict(name=name, codes=rng.integers(0, 5, L).astype(np.uint8), qual=rng.integers(33, 127, L).astype(np.uint8),
                comment=("" if i % 4 == 3 else f"BC:Z:{'x' * (i % 23)} c{i}"), recs=recs, fin_status=fin_status)


def _edge_reads():
    rng = np.random.default_rng(20)
    reads = []

    def add(L, recs, **kw):
        reads.append(_read(rng, len(reads), L, recs, **kw))
    for L in LENGTHS:                                                 # one record, then none, at every length
        add(L, [_rec(rng, L, 0)])
        add(L, [])
    # numbers at their digit boundaries; a contig whose offset is beyond 2^32; 2^31 - 2 needs a long contig
    for pos1, rid, mapq, nm in ((9, 0, 0, 0), (10, 1, 9, 100), (99_999_999, 2, 10, 0), ((1 << 31) - 2, 2, 60, 100),
                                (1, 3, 60, 9), (999, 4, 59, 10), (1000, 3, 1, 99)):
        add(100, [_rec(rng, 100, 0, pos1=pos1, rid=rid, mapq=mapq, NM=nm)])
    add(64, [_rec(rng, 64, 0, n_words=1, clip5=0, clip3=0, md="64")])                    # CIGAR of one word, MD of one byte ...
    add(17, [_rec(rng, 17, 0, n_words=1, clip5=0, clip3=0, md="0")])
    add(1024, [_rec(rng, 1024, 0, n_words=200, clip5=20, clip3=31, md="A7" * 512)])     # ... of 200 words, MD of 1 KB
    add(1024, [_rec(rng, 1024, 0, n_words=200, clip5=0, clip3=0, md="9" * 1024), _rec(rng, 1024, 1, n_words=130, clip5=5,
                                                                                      clip3=0)])
    for n_rec in (3, 8):                                              # primaries on both strands, clips at both ends
        for L in (65, 256):
            recs = [_rec(rng, L, k, is_rev=k & 1, clip5=3 + k, clip3=1 + 2 * k) for k in range(n_rec)]
            add(L, recs)
            recs = [_rec(rng, L, k, is_rev=(k + 1) & 1, clip5=(k % 3) * 4, clip3=((k + 1) % 3) * 5) for k in range(n_rec)]
            add(L, recs)
    # a 0x100 record between primaries; a secondary alone behind a primary; 0x10000; xs -1
    add(100, [_rec(rng, 100, 0), _rec(rng, 100, 1, flag=0x100, xs=-1, mapq=0), _rec(rng, 100, 2)])
    add(100, [_rec(rng, 100, 0), _rec(rng, 100, 1, flag=0x100, xs=-1, mapq=0)])
    add(100, [_rec(rng, 100, 0, xs=-1), _rec(rng, 100, 1, flag=0x10000), _rec(rng, 100, 2, flag=0x10000, xs=-1)])
    add(33, [_rec(rng, 33, 0)], name="n" * 255)
    # the four causes of SMEM_SAM_HOST, each between untouched neighbours
    add(50, [_rec(rng, 50, 0), S.Rec(status=4, rid=-1, pos=-1, mapq=3, flag=0x800, score=40, xs=0)])
    add(40, [_rec(rng, 40, 0)])
    add(50, [_rec(rng, 50, 0, mapq=-1), _rec(rng, 50, 1, mapq=-1)])
    add(41, [])
    add(50, [_rec(rng, 50, 0)], fin_status=1)
    add(42, [_rec(rng, 42, 0), _rec(rng, 42, 1)])
    add(0, [])
    add(43, [_rec(rng, 43, 0)])
    for st in (1, 2, 3):
        add(30, [S.Rec(status=st, rid=-1, pos=-1, mapq=0, flag=0, score=35, xs=0)])
    return reads


def _many_reads(n=5000):
    rng = np.random.default_rng(21)
    reads = []
    for i in range(n):
        L = int(rng.integers(1, 90))
        k = int(rng.integers(0, 4)) if L >= 8 else int(rng.integers(0, 2))
        reads.append(_read(rng, i, L, [_rec(rng, L, j) for j in range(k)]))
    return reads


def _pack(reads):
    from smemgpu.lib import ALN_DT, SAM_REC_DT
    lens = [r["codes"].size for r in reads]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    recs = [x for r in reads for x in r["recs"]]
    aln_off = np.concatenate([[0], np.cumsum([len(r["recs"]) for r in reads])]).astype(np.uint64)
    alns = np.zeros(len(recs), dtype=ALN_DT)
    rid = np.zeros(len(recs), dtype=np.int32)
    sr = np.zeros(len(recs), dtype=SAM_REC_DT)
    cig, md = [np.zeros(3, np.uint32)], [b"###"]                      # (the pools do not start at a record)
    nc, nm = 3, 3
    for k, x in enumerate(recs):
        alns[k] = (x.pos, x.is_rev, len(x.cigar), x.NM, 0, 1, x.status, nc, nm, len(x.md), 0)
        rid[k] = x.rid
        sr[k] = (x.mapq, x.flag, x.score, x.xs)
        cig.append(np.array(x.cigar, dtype=np.uint32))
        md.append(x.md.encode())
        nc += len(x.cigar)
        nm += len(x.md)
    e = np.zeros(0, np.uint8)
    return dict(codes=np.concatenate([r["codes"] for r in reads] + [e]), offs=offs,
                quals=np.concatenate([r["qual"] for r in reads] + [e]), names=[r["name"] for r in reads],
                comments=[r["comment"] for r in reads], aln_off=aln_off, alns=alns, rid=rid, recs=sr,
                cigar=np.concatenate(cig).astype(np.uint32), md=np.frombuffer(b"".join(md), dtype=np.uint8),
                fin_status=np.array([r["fin_status"] for r in reads], dtype=np.int32))


def _want(reads, qual=True, comments=True, rg_id=None):
    return [S.read_text(r["name"], r["codes"], r["qual"] if qual else None, r["comment"] if comments else None,
                        CTG_NAMES, CTG_OFFS, r["recs"], rg_id, r["fin_status"]) for r in reads]


def _call(gpu, A, qual=True, comments=True, rg_id=None, **kw):
    return gpu.sam_text(A["codes"], A["offs"], A["names"], A["quals"] if qual else None,
                        A["comments"] if comments else None, A["aln_off"], A["alns"], A["rid"], A["recs"], A["cigar"],
                        A["md"], CTG_OFFS, CTG_NAMES, fin_status=A["fin_status"], rg_id=rg_id, **kw)


def _same(got, want):
    from smemgpu.lib import SAM_HOST
    assert got.text_off.size == len(want) + 1 and got.text_off[0] == 0
    for r, w in enumerate(want):
        assert got.status[r] == (SAM_HOST if w is None else 0), r
        assert got.read(r) == (w or b""), (r, got.read(r), w)
    assert int(got.text_off[-1]) == got.text.size == sum(len(w) for w in want if w)


@pytest.fixture(scope="module")
def edge():
    reads = _edge_reads()
    return reads, _pack(reads)


def test_edge_shapes_cover_every_alignment(edge):
    """the fixture itself: every start offset mod 16 occurs for a record's first byte, SEQ and QUAL"""
    reads, _A = edge
    want = _want(reads)
    at, first, seq, qual = 0, set(), set(), set()
    for w in want:
        for line in (w or b"").split(b"\n")[:-1]:
            f = line.split(b"\t")
            first.add(at % 16)
            if f[9] != b"*":
                s = at + sum(len(x) + 1 for x in f[:9])
                seq.add(s % 16)
                qual.add((s + len(f[9]) + 1) % 16)
            at += len(line) + 1
    assert first == seq == qual == set(range(16))
    assert {r["codes"].size for r in reads} >= set(LENGTHS) and max(len(r["name"]) for r in reads) == 255
    assert {len(r["name"]) for r in reads} >= set(range(1, 41))
    assert sum(w is None for w in want) == 7 and max(len(r["recs"]) for r in reads) == 8


@pytest.mark.parametrize("qual,comments,rg_id", [(True, True, "grp1"), (True, False, None), (False, True, None),
                                                 (False, False, "a-long-read-group.id")])
def test_host_call_edge_shapes(handles, edge, qual, comments, rg_id):
    reads, A = edge
    got = _call(handles("g2"), A, qual, comments, rg_id)
    _same(got, _want(reads, qual, comments, rg_id))
    assert got.kernel_ms > 0


def test_host_call_host_reads_and_neighbours(handles, edge):
    """each cause of SMEM_SAM_HOST gives zero bytes and leaves the reads around it as they are"""
    from smemgpu.lib import SAM_HOST
    reads, A = edge
    got, want = _call(handles("g2"), A), _want(reads)
    host = [r for r, w in enumerate(want) if w is None]
    causes = set()
    for r in host:
        x = reads[r]
        causes.add("status" if any(y.status for y in x["recs"]) else "mapq" if any(y.mapq == -1 for y in x["recs"])
                   else "fin" if x["fin_status"] else "empty")
        assert got.status[r] == SAM_HOST and got.text_off[r] == got.text_off[r + 1]
        for q in (r - 1, r + 1):
            if 0 <= q < len(reads) and want[q] is not None:
                assert got.read(q) == want[q]
    assert causes == {"status", "mapq", "fin", "empty"}


def test_host_call_many_reads_and_capacity(handles):
    """5000 reads: the write kernel's grid takes reads in turn; SMEM_E_CAPACITY reports the size a
    retry needs and the retry succeeds; an empty read list"""
    import smemgpu
    from smemgpu import lib as L
    gpu = handles("g2")
    reads = _many_reads()
    assert len(reads) > 4096                                          # SAM_WRITE_BLOCKS_MAX
    A, want = _pack(reads), _want(reads)
    total = sum(len(w) for w in want if w)
    with pytest.raises(smemgpu.SmemError, match="SMEM_E_CAPACITY") as e:
        _call(gpu, A, text_cap=total - 1, grow=False)
    assert e.value.n_bytes == total
    _same(_call(gpu, A, text_cap=total, grow=False), want)
    _same(_call(gpu, A, text_cap=16), want)                           # the binding's own retry
    none = _pack([])
    got = _call(gpu, none)
    assert got.text.size == 0 and got.text_off.tolist() == [0] and got.status.size == 0
    assert gpu.fault()[0] == 0
    assert L.FETCH_ALL == 15


def test_order_and_contract(handles):
    import smemgpu
    from oracle import oracle
    from smemgpu.lib import FETCH_ALN, FETCH_FIN, FETCH_SAM
    import regfin_data as D
    name = "g2_r4_default"
    F, want = SD.load(name), SD.texts(name)
    gpu = handles("g2")
    b = _to_reg2aln(gpu, F, text=False, finalize=False)
    try:
        b.reg_finalize(ids=F["ids"])
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
            b.sam()                                                   # before reg2aln
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
            b.fetch(FETCH_SAM)                                        # before the stage
        fin = b.fetch(FETCH_FIN).fin
        b.reg2aln(_opt(), fin.sel_idx, fin.sel_off)
        b.set_read_text(F["names"], F["quals"])
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
            b.sam()                                                   # reg2aln over the caller's index lists
        b.reg2aln(_opt())
        b.set_reads(F["reads"].codes, F["reads"].offs)                # a later set_reads ends the read text
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
            b.sam()
    finally:
        b.close()
    b = _to_reg2aln(gpu, F, text=False)
    try:
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
            b.sam()                                                   # without read text
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
            b.set_read_text(["n" * 256] + F["names"][1:], F["quals"])
        b.set_read_text(F["names"], F["quals"])
        mem0 = b.memory()
        b.sam()
        mem1 = b.memory()
        first = b.fetch(FETCH_SAM | FETCH_ALN)
        mem2 = b.memory()
        b.sam()
        assert mem1[0] > mem0[0] and b.memory()[0] == mem2[0] == mem1[0]    # the stage's buffers: first call only
        again = b.fetch(FETCH_SAM).sam
        assert again.text.tobytes() == first.sam.text.tobytes() == b"".join(t for t in want if t is not None)
        assert np.array_equal(again.text_off, first.sam.text_off) and first.aln is not None
        b.sam("rg7")                                                  # the read-group id reaches every line
        rg = b.fetch(FETCH_SAM).sam
        assert rg.text.tobytes().count(b"\tRG:Z:rg7") == rg.text.tobytes().count(b"\n") > 0
        b.set_read_text(F["names"])                                   # no qualities: '*'
        b.sam()
        nq = b.fetch(FETCH_SAM).sam
        ctg_names, ctg_offs, _l = X.table(F["contigs"])
        r0 = next(r for r, t in enumerate(want) if t is not None)
        assert nq.read(r0) == S.read_text(F["names"][r0], F["reads"].read(r0), None, None, ctg_names, ctg_offs,
                                          SD.records(name)[r0])
        b.reg_finalize(ids=F["ids"])                                  # a later reg_finalize ends the results
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
            b.fetch(FETCH_SAM)
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
            b.sam()
        b.reg2aln(_opt())
        b.sam()
        b.reg2aln(_opt())                                             # and so does a later reg2aln
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
            b.fetch(FETCH_SAM)
        b.sam()
        b.chain2aln(oracle.aln_opt())                                 # and a later chain2aln
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
            b.fetch(FETCH_SAM)
        assert gpu.fault()[0] == 0
    finally:
        b.close()
    # names need a table of as many contigs; a handle without names or without a table refuses the stage
    names, offs, lens = X.table(D.contigs("g2"))
    with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
        gpu.load_contig_names(names + ["one_more"])
    gpu.load_contigs(offs, lens, F["l_pac"])                          # a new table drops the names
    b = _to_reg2aln(gpu, F)
    try:
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
            b.sam()
        gpu.load_contig_names(names)
        gpu.load_contig_names(names)                                  # (loading again replaces them)
        b.sam()
        assert b.fetch(FETCH_SAM).sam.text.tobytes() == b"".join(t for t in want if t is not None)
    finally:
        b.close()


def test_reserved_slot_carries_the_stage(handles):
    """once the stage has run on a handle, smem_gpu_reserve_slots sizes a worker slot for it: the
    read text and the stage then run on the slot's batch (smem_gpu_collect_ex) without growing it,
    same text"""
    import ctypes as C
    import smemgpu
    from oracle import oracle
    from smemgpu.lib import FETCH_SAM, ChainOptT, COLLECT_NO_FETCH, SamOptT, pack_strings
    from test_gpu_product import _collect
    name, n = "g2_r4_default", 64
    F, want = SD.load(name), SD.texts(name)
    reads = F["reads"]
    gpu = handles("g2")
    b = _to_reg2aln(gpu, F)
    try:
        b.sam()                                             # the handle has seen the stage
    finally:
        b.close()
    lib = smemgpu.load()
    gpu.reserve_slots(1, n, int(reads.lens.max()))
    rc, bh, _keep = _collect(lib, gpu._h, 0, reads, 0, n, flags=COLLECT_NO_FETCH)   # (waits for its slot)
    assert rc == 0
    assert lib.smem_batch_sa(bh, 19, 10000) == 0
    co = ChainOptT(100, 10000, 0.5, 0.5, 1)
    assert lib.smem_batch_chain(bh, F["l_pac"], C.byref(co)) == 0
    ao, fo, o, so = oracle.aln_opt(), smemgpu.fin_opt(), _opt(), SamOptT(None)
    assert lib.smem_batch_chain2aln(bh, C.byref(ao)) == 0
    ids = np.ascontiguousarray(F["ids"][:n], dtype=np.int64)
    assert lib.smem_batch_reg_finalize(bh, ids.ctypes.data, 0, C.byref(fo)) == 0
    assert lib.smem_batch_reg2aln(bh, C.byref(o), None, None) == 0
    d0, d1 = C.c_uint64(), C.c_uint64()
    assert lib.smem_batch_memory(bh, C.byref(d0), None) == 0
    nm, nm_off = pack_strings(F["names"][:n])
    q = np.ascontiguousarray(F["quals"][:int(reads.offs[n])])
    assert lib.smem_batch_set_read_text(bh, nm.ctypes.data, nm_off.ctypes.data, q.ctypes.data, None, None) == 0
    assert lib.smem_batch_sam(bh, C.byref(so)) == 0
    assert lib.smem_batch_memory(bh, C.byref(d1), None) == 0
    assert d1.value == d0.value                             # the stage's buffers came with the slot
    assert lib.smem_batch_fetch_mask(bh, FETCH_SAM) == 0
    tx, to, ts, tb = C.c_void_p(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_int32)(), C.c_uint64()
    assert lib.smem_batch_sam_results(bh, C.byref(tx), C.byref(to), C.byref(ts), C.byref(tb)) == 0
    text = C.string_at(tx.value, int(tb.value))
    assert int(to[n]) == len(text) and text == b"".join(t for t in want[:n] if t is not None) and len(text) > 0
    assert [int(ts[r]) for r in range(n)] == [int(t is None) for t in want[:n]]


_CHILD = r"""
import os, sys
import numpy as np
import smemgpu
from smemgpu.lib import FETCH_ALN, FETCH_SAM
import samtext_data as SD, xref_ref as X, regfin_data as D, test_gpu_samtext as G
from tests import golden_data
import tempfile

name = "g2_r4_default"
F, want = SD.load(name), SD.texts(name)
paths = golden_data.files("g2", tempfile.mkdtemp())
gpu = smemgpu.Gpu(smemgpu.Index.read(paths["bwt"]), device=int(sys.argv[1]))
gpu.load_sa(smemgpu.SA.read(paths["sa"]))
gpu.load_pac(golden_data.pac("g2"), golden_data.l_pac("g2"))
names, offs, lens = X.table(D.contigs("g2"))
gpu.load_contigs(offs, lens, golden_data.l_pac("g2"))
gpu.load_contig_names(names)
b = G._to_reg2aln(gpu, F)
aln0 = b.fetch(FETCH_ALN).aln
os.environ["SMEM_GPU_FAIL"] = sys.argv[2]
try:
    b.sam()
    raise SystemExit("the injected failure did not surface")
except smemgpu.SmemError as e:
    assert "SMEM_E_DEVICE" in str(e) and "injected" in str(e), e
os.environ.pop("SMEM_GPU_FAIL")
assert gpu.fault()[0] == 0
try:
    b.fetch(FETCH_SAM)
    raise SystemExit("results of a failed call were fetchable")
except smemgpu.SmemError as e:
    assert "SMEM_E_ARG" in str(e), e
aln1 = b.fetch(FETCH_ALN).aln                     # the earlier stage's results stay
assert aln1.alns.tobytes() == aln0.alns.tobytes() and aln0.alns.size
b.sam()
sam = b.fetch(FETCH_SAM).sam
b.close()
gpu.close()
assert sam.text.tobytes() == b"".join(t for t in want if t is not None)
print("child ok", sam.text.size)
"""


def test_injected_failure_in_a_child(gpu_device, built):
    """SMEM_GPU_FAIL=sam:1 (the library's own return-code hook, after the work is enqueued): the
    call returns SMEM_E_DEVICE, the alignments stay fetchable, the next call succeeds and equals
    the restatement.  No GPU fault is provoked."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "bwa-mem-harp2_amd"), ROOT,
                                                       os.path.join(ROOT, "tests")]))
    env.pop("SMEM_GPU_FAIL", None)
    p = subprocess.run([sys.executable, "-c", _CHILD, str(gpu_device), "sam:1"], capture_output=True, timeout=120,
                       env=env)
    out = p.stdout.decode(errors="replace") + p.stderr.decode(errors="replace")
    assert p.returncode == 0 and "child ok" in out, out[-3000:]
