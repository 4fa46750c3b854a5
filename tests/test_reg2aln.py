"""Regions -> alignments: the alignment part of mem_reg2aln
(software/bwamem.c:1481-1553) -- infer_bw, the band-doubling loop over
bwa_gen_cigar2 / ksw_global2 with traceback, NM / MD, the edge-deletion squeeze
and the clips -- on the GPU (smem_reg2aln, Gpu.reg2aln).

Bar: exact.  tests/reg2aln_ref.py restates the stage in Python; it is pinned,
without a GPU, to the reference's own SAM records over the reference's own
regions (tests/golden/cigar/, made by tests/golden/make_golden_cigar.py).  The
GPU is then checked against those records, and against the restatement where
no record speaks (score, tries, status, unmatched regions, synthetic shapes).
"""
import ctypes as C
import functools
import gzip
import hashlib
import json
import os
import re

import numpy as np
import pytest

import reg2aln_ref as ref
from tests import golden_data

CIGAR_DIR = os.path.join(golden_data.GOLDEN, "cigar")
MAX_UNMATCHED = 0.02


# ------------------------------------------------------------------ fixtures
def _blob(g, ext, man):
    with gzip.open(os.path.join(CIGAR_DIR, f"{g}.{ext}.gz"), "rb") as fh:
        data = fh.read()
    assert hashlib.sha256(data).hexdigest() == man[g]["sha256"][ext], "fixture corrupted"
    return data


def _contigs(g):
    """contig name -> offset in the concatenated forward strand"""
    out, name, off, n = {}, None, 0, 0
    for line in golden_data.gz(f"{g}.fa.gz").split(b"\n"):
        if line.startswith(b">"):
            if name is not None:
                out[name] = off
                off += n
            name, n = line[1:].split()[0].decode(), 0
        else:
            n += len(line.strip())
    out[name] = off
    return out


def _sam_ops(s):
    """SAM CIGAR -> smem_aln_t words; a supplementary record's H is mem_aln2sam's
    print of the clip mem_reg2aln made (op 3)"""
    return tuple(int(n) << 4 | (3 if op == "H" else "MIDS".index(op)) for n, op in re.findall(r"(\d+)([MIDSH])", s))


@functools.lru_cache(maxsize=None)
def _fixture(g):
    from smemgpu import synth
    with open(os.path.join(CIGAR_DIR, "manifest.json")) as fh:
        man = json.load(fh)
    data = _blob(g, "smrd", man)
    import struct
    n, nb = struct.unpack_from("<QQ", data, 8)
    lens = np.frombuffer(data, dtype="<i4", count=n, offset=24).astype(np.int32)
    codes = np.frombuffer(data, dtype=np.uint8, count=nb, offset=24 + 4 * n).copy()
    reads = synth.Reads(lens, codes, np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]))
    regs, reg_off = golden_data.smrg_parse(_blob(g, "smrg", man))
    recs = []
    for line in _blob(g, "tsv", man).decode().split("\n"):
        if line:
            f = line.split("\t")
            recs.append((f[0], int(f[1]), f[2], int(f[3]), f[4], int(f[5]), f[6]))
    l_pac = golden_data.l_pac(g)
    ctg = _contigs(g)
    # a record belongs to the region of its read with its geometry: strand, clips,
    # contig-relative position and reference length -- nothing else
    hits = []
    for qname, flag, rname, pos, cigar, _nm, _md in recs:
        r, ops, rev = int(qname[1:]), _sam_ops(cigar), bool(flag & 16)
        c5 = ops[0] >> 4 if ops[0] & 0xf == 3 else 0
        c3 = ops[-1] >> 4 if ops[-1] & 0xf == 3 and len(ops) > 1 else 0
        rlen = sum(c >> 4 for c in ops if c & 0xf in (0, 2))
        gpos, L, hit = ctg[rname] + pos - 1, int(lens[r]), -1
        for k in range(int(reg_off[r]), int(reg_off[r + 1])):
            rb, re_, qb, qe = (int(regs[k][f]) for f in ("rb", "re", "qb", "qe"))
            if rb < 0 or re_ < 0 or (rb < l_pac) == rev:
                continue
            if ((L - qe, qb) if rev else (qb, L - qe)) == (c5, c3) and (2 * l_pac - re_ if rev else rb) == gpos \
                    and re_ - rb == rlen:
                hit = k
                break
        hits.append(hit)
    return dict(man=man[g], reads=reads, regs=regs, reg_off=reg_off, recs=recs, hits=hits, l_pac=l_pac,
                pac=golden_data.pac(g))


def _read_of_region(reg_off):
    return np.repeat(np.arange(reg_off.size - 1), np.diff(reg_off.astype(np.int64)))


@functools.lru_cache(maxsize=None)
def _fixture_ref(g):
    """the restatement over every region of the fixture (computed once)"""
    F = _fixture(g)
    rd = _read_of_region(F["reg_off"])
    return [ref.reg2aln(ref.Opt(), F["l_pac"], F["pac"], F["reads"].read(int(rd[k])), F["regs"][k])
            for k in range(F["regs"].size)]


def _record_tuple(rec, ctg_off):
    _q, flag, rname, pos, cigar, nm, md = rec
    return (int(bool(flag & 16)), ctg_off[rname] + pos - 1, _sam_ops(cigar), nm, md)


@pytest.mark.parametrize("g", ["g1", "g2"])
def test_restatement_vs_reference_records(g):
    """The Python restatement over the reference's regions gives every matched SAM
    record of the reference: strand, position, CIGAR with clips, NM and MD, no
    tolerance; at most 2 % of the mapped records have no region of their geometry."""
    F = _fixture(g)
    want_man = F["man"]
    assert len(F["recs"]) == want_man["records"] and F["regs"].size == want_man["regions"]
    n_un = sum(1 for h in F["hits"] if h < 0)
    assert n_un <= MAX_UNMATCHED * len(F["recs"]), f"{n_un} of {len(F['recs'])} records without a region"
    assert len(F["recs"]) - n_un == want_man["matched"]
    got = _fixture_ref(g)
    ctg = _contigs(g)
    gapped = 0
    for rec, h in zip(F["recs"], F["hits"]):
        if h < 0:
            continue
        a = got[h]
        assert a.status == 0
        assert (a.is_rev, a.pos, a.cigar, a.NM, a.md) == _record_tuple(rec, ctg), (rec, a)
        gapped += bool(re.search("[ID]", rec[4]))
    assert gapped == want_man["matched_gapped"] and gapped >= 300


# --------------------------------------------------------------- GPU helpers
def _got(alns, cigar, md, k):
    a = alns[k]
    co, mo = int(a["cigar_off"]), int(a["md_off"])
    return ref.Aln(pos=int(a["pos"]), is_rev=int(a["is_rev"]),
                   cigar=tuple(int(c) for c in cigar[co:co + int(a["n_cigar"])]), NM=int(a["NM"]),
                   score=int(a["score"]), tries=int(a["tries"]), status=int(a["status"]),
                   md=md[mo:mo + int(a["md_len"])].tobytes().decode())


def _gpu_for(genome_codes, device):
    import smemgpu
    return smemgpu.Gpu(smemgpu.Index.build(genome_codes), device=device)


def _pack(codes):
    c = np.concatenate([codes, np.zeros((-codes.size) % 4, np.uint8)]).reshape(-1, 4).astype(np.uint8)
    return (c[:, 0] << 6 | c[:, 1] << 4 | c[:, 2] << 2 | c[:, 3]).astype(np.uint8)


def _c_opt(o: ref.Opt):
    import smemgpu
    c = smemgpu.aln_opt(a=o.a, w=o.w, o_del=o.o_del, e_del=o.e_del, o_ins=o.o_ins, e_ins=o.e_ins)
    for i, row in enumerate(o.mat()):
        for j, v in enumerate(row):
            c.mat[i * 5 + j] = v
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("resident", [False, True], ids=["explicit_pac", "resident_pac"])
@pytest.mark.parametrize("g", ["g1", "g2"])
def test_reg2aln_gpu_fixture(gpu_device, g, resident):
    """Every matched region equals the reference's record in (is_rev, pos, CIGAR with
    clips, NM, MD); every region equals the restatement in all fields."""
    import smemgpu
    import tempfile
    F = _fixture(g)
    want = _fixture_ref(g)
    with tempfile.TemporaryDirectory() as d:
        idx = smemgpu.Index.read(golden_data.files(g, d)["bwt"])
    gpu = smemgpu.Gpu(idx, device=gpu_device)
    try:
        if resident:
            gpu.load_pac(F["pac"], F["l_pac"])
        alns, cigar, md, ms = gpu.reg2aln(None if resident else F["pac"], F["l_pac"], F["reads"].codes,
                                          F["reads"].offs, F["regs"], F["reg_off"], _c_opt(ref.Opt()))
    finally:
        gpu.close()
    print(f"reg2aln {g}: {F['regs'].size} regions, kernel {ms:.3f} ms")
    assert alns.size == F["regs"].size
    ctg = _contigs(g)
    for rec, h in zip(F["recs"], F["hits"]):
        if h >= 0:
            a = _got(alns, cigar, md, h)
            assert (a.is_rev, a.pos, a.cigar, a.NM, a.md) == _record_tuple(rec, ctg), (rec, a)
    for k in range(alns.size):
        assert _got(alns, cigar, md, k) == want[k], (k, F["regs"][k])


# ------------------------------------------------------- synthetic regions
G_LEN = 24_000
RUN_AT, RUN_LEN = 12_000, 12     # a planted homopolymer (A) run


@functools.lru_cache(maxsize=None)
def _genome():
    rng = np.random.default_rng(77)
    g = rng.integers(0, 4, size=G_LEN, dtype=np.uint8)
    g[RUN_AT:RUN_AT + RUN_LEN] = 0
    g[RUN_AT - 1], g[RUN_AT + RUN_LEN] = 1, 2
    g[200:205] = [0, 1, 1, 1, 1]     # 1 x 5 regions: the single M first, last, nowhere
    g[300:305] = [1, 1, 1, 1, 0]
    g[400:405] = 2
    return g


class _Builder:
    def __init__(self):
        self.reads, self.regs, self.off, self.tags = [], [], [0], []

    def read(self, codes, regions, tag):
        """regions: (rb, re, qb, qe, truesc, w) in doubled coordinates"""
        self.reads.append(np.asarray(codes, dtype=np.uint8))
        for r in regions:
            self.regs.append(r)
            self.tags.append(tag)
        self.off.append(len(self.regs))

    def one(self, query, p, tlen, rev, truesc, w, tag, clip=(0, 0)):
        """one region over genome[p, p + tlen) for `query` (given on the forward
        strand; reverse-complemented into the read when rev), clip = (5', 3')
        extra read bases outside the region"""
        L = G_LEN
        q = np.asarray(query, dtype=np.uint8)
        if rev:
            q = np.where(q < 4, 3 - q, 4).astype(np.uint8)[::-1]
            rb, re_ = 2 * L - (p + tlen), 2 * L - p
        else:
            rb, re_ = p, p + tlen
        rd = np.concatenate([np.full(clip[0], 1, np.uint8), q, np.full(clip[1], 2, np.uint8)])
        self.read(rd, [(rb, re_, clip[0], clip[0] + q.size, truesc, w)], tag)

    def arrays(self):
        from smemgpu import synth
        lens = np.array([r.size for r in self.reads], dtype=np.int32)
        reads = synth.Reads(lens, np.concatenate(self.reads), np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]))
        regs = np.zeros(len(self.regs), dtype=golden_data.ALNREG_DT)
        for k, (rb, re_, qb, qe, truesc, w) in enumerate(self.regs):
            regs[k]["rb"], regs[k]["re"], regs[k]["qb"], regs[k]["qe"] = rb, re_, qb, qe
            regs[k]["truesc"], regs[k]["w"], regs[k]["score"] = truesc, w, truesc
        return reads, regs, np.array(self.off, dtype=np.uint64)


def _truesc_for_w2(l, w2):
    """the truesc at which infer_bw (a 1, gaps 6 + 1) asks for band w2 >= 1 on
    sequences whose shorter side is l (software/bwamem.c:1198)"""
    return l - 4 - w2


# the band widths and column counts wanted: lane-group boundaries (16, 32, 64) and a
# row of several 64-column passes
N_COLS = [15, 16, 17, 31, 32, 33, 63, 64, 65, 129]


@functools.lru_cache(maxsize=None)
def _synthetic(big: bool):
    g = _genome()
    B = _Builder()
    rng = np.random.default_rng(5)
    sub = lambda s, i: (int(s[i]) + 1) & 3   # noqa: E731
    for rev in (False, True):
        s = "r" if rev else "f"
        # 1 x 1, and 1 x 5: all deletion plus one M (the squeeze moves pos or drops the tail)
        B.one(g[100:101], 100, 1, rev, 1, 0, "1x1" + s)
        B.one(g[200:201], 200, 5, rev, 1, 10, "1x5trail" + s)
        B.one(g[304:305], 300, 5, rev, 1, 10, "1x5lead" + s)
        B.one([3], 400, 5, rev, 0, 10, "1x5mm" + s, clip=(3, 2))
        # equal lengths: perfect (w2 = 0, no DP) and with one mismatch
        q = g[1000:1120].copy()
        B.one(q, 1000, 120, rev, 120, 5, "perfect" + s)
        q[60] = sub(q, 60)
        B.one(q, 1000, 120, rev, 115, 5, "one_mm" + s, clip=(7, 0))
        # odd column counts through truesc (w2 = w), on near-perfect reads with a 2-base deletion
        for n_col in (15, 17, 31, 33, 63, 65, 129):
            w, l = (n_col - 1) // 2, 150 if n_col < 129 else 300
            p = 2000 + 31 * n_col
            q = np.concatenate([g[p:p + 70], g[p + 72:p + l + 2]])
            B.one(q, p, l + 2, rev, _truesc_for_w2(l, w), w, f"ncol{n_col}" + s, clip=(0, 4))
        # even column counts: qlen columns, the band opened by a deletion of d bases (min_w = d + 3)
        for n_col, d in ((16, 6), (32, 13), (64, 29)):
            p = 7000 + 101 * n_col
            q = np.concatenate([g[p:p + n_col // 2], g[p + n_col // 2 + d:p + n_col + d]])
            B.one(q, p, n_col + d, rev, n_col - 6 - d, 100, f"ncol{n_col}" + s)
        # a 12-base insertion and, later, a 12-base deletion at w2 = 8 (the least infer_bw gives
        # equal lengths): the first band cannot hold them, the second can, the third confirms
        p = 9000
        q = np.concatenate([g[p:p + 50], rng.integers(0, 4, 12, dtype=np.uint8), g[p + 50:p + 100], g[p + 112:p + 150]])
        B.one(q, p, 150, rev, _truesc_for_w2(150, 8), 100, "three_tries" + s)
        # infer_bw above opt->w: the region's own w clamps it
        q = np.concatenate([g[9500:9560], g[9564:9650]])
        B.one(q, 9500, 150, rev, 20, 9, "w_clamp" + s)
        # one base less than the planted A run: the gap must land leftmost on the forward strand
        p = RUN_AT - 60
        q = np.concatenate([g[p:RUN_AT + 5], g[RUN_AT + 6:p + 150]])
        q[100] = sub(q, 100)
        B.one(q, p, 150, rev, 130, 20, "homopolymer_del" + s)
        q = np.concatenate([g[p:RUN_AT + 5], [0], g[RUN_AT + 5:p + 149]]).astype(np.uint8)
        B.one(q, p, 149, rev, 130, 20, "homopolymer_ins" + s, clip=(2, 3))
        # N at a mismatch and at the edges of a gap
        p = 10500
        q = np.concatenate([g[p:p + 80], g[p + 85:p + 155]])
        q[30], q[79], q[80] = 4, 4, 4
        B.one(q, p, 155, rev, 125, 20, "n_del" + s)
        q = np.concatenate([g[p:p + 80], [4, 1, 2, 4], g[p + 80:p + 146]]).astype(np.uint8)
        q[10] = 4
        B.one(q, p, 146, rev, 125, 20, "n_ins" + s)
    if big:  # the scratch tier: 1000 x 1040 at w = 200 (a 201-byte row, 209 KB of directions)
        p = 13000
        q = np.concatenate([g[p:p + 500], g[p + 540:p + 1040]])
        for i in range(40, 1000, 97):
            q[i] = sub(q, i)
        B.one(q, p, 1040, False, _truesc_for_w2(1000, 200), 200, "big")
    # unmapped, bridging l_pac and past the limits, each between two good neighbours
    L = G_LEN
    q = g[15000:15150]
    good = (15000, 15150, 0, 150, 150, 5)
    B.read(q, [good, (-1, 15150, 0, 150, 150, 5), good, (L - 70, L + 80, 0, 150, 150, 5), good,
               (15150, 15000, 0, 150, 150, 5), good, (15000, 15150, 40, 40, 150, 5), good], "status")
    q = g[16000:17100]
    good = (16000, 16100, 0, 100, 100, 5)
    B.read(q, [good, (16000, 17025, 0, 1025, 1025, 5), good, (16000, 16000 + 2049, 0, 1000, 900, 5), good],
           "limits")
    reads, regs, reg_off = B.arrays()
    return reads, regs, reg_off, tuple(B.tags)


OPTS = {
    "default": ref.Opt(),
    "a2": ref.Opt(a=2, b=8, o_del=12, e_del=2, o_ins=12, e_ins=2),
    "o_ins0": ref.Opt(o_ins=0),
}


@functools.lru_cache(maxsize=None)
def _synthetic_ref(name):
    reads, regs, reg_off, _tags = _synthetic(name == "default")
    rd = _read_of_region(reg_off)
    pac = _pack(_genome())
    return [ref.reg2aln(OPTS[name], G_LEN, pac, reads.read(int(rd[k])), regs[k]) for k in range(regs.size)]


def _n_col(o, reg):
    """columns of the region's first try (0: no DP), by the restated classifier"""
    return ref.classify(o, reg, 1).n_col[0]


def test_synthetic_regions_hit_their_shapes():
    """The synthetic set reaches what it is there for (judged by the restatement):
    every wanted column count on both strands, the no-DP branch, three tries, the
    squeeze on either side, a leftmost gap in the homopolymer, every status."""
    reads, regs, reg_off, tags = _synthetic(True)
    want = _synthetic_ref("default")
    by = {t: k for k, t in enumerate(tags) if t not in ("status", "limits")}
    o = OPTS["default"]
    for s in "fr":
        for n in N_COLS:
            assert _n_col(o, regs[by[f"ncol{n}{s}"]]) == n, (n, s)
            assert want[by[f"ncol{n}{s}"]].tries == 1 and re.search("D", ref.cigar_str(want[by[f"ncol{n}{s}"]].cigar))
        assert _n_col(o, regs[by["perfect" + s]]) == 0 and _n_col(o, regs[by["one_mm" + s]]) == 0
        assert want[by["one_mm" + s]].NM == 1 and want[by["one_mm" + s]].score == 115
        assert want[by["three_tries" + s]].tries == 3
        assert want[by["w_clamp" + s]].tries == 1 and _n_col(o, regs[by["w_clamp" + s]]) == 19
        for t in ("1x5lead", "1x5trail"):
            a = want[by[t + s]]
            assert ref.cigar_str(a.cigar) == "1M" and a.NM == 0 and a.md == "1"
        lead, trail = want[by["1x5lead" + s]], want[by["1x5trail" + s]]
        assert (lead.pos, trail.pos) == (304, 200)
        # the deleted / inserted A sits at the run's first base on the forward strand, whichever strand was read
        a = want[by["homopolymer_del" + s]]
        assert ref.cigar_str(a.cigar) == "60M1D89M" and "^A" in a.md and a.pos == RUN_AT - 60
        a = want[by["homopolymer_ins" + s]]
        assert ref.cigar_str(a.cigar) == ("3S60M1I89M2S" if s == "r" else "2S60M1I89M3S")
        assert "N" not in want[by["n_del" + s]].md and want[by["n_del" + s]].NM >= 8
    assert _n_col(o, regs[by["big"]]) == 401 and want[by["big"]].tries == 1
    st = [a.status for k, a in enumerate(want) if tags[k] == "status"]
    assert st == [0, ref.UNMAPPED, 0, ref.NOCIGAR, 0, ref.NOCIGAR, 0, ref.NOCIGAR, 0]
    st = [a.status for k, a in enumerate(want) if tags[k] == "limits"]
    assert st == [0, ref.REJECT, 0, ref.REJECT, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(OPTS))
def test_reg2aln_gpu_synthetic(gpu_device, name):
    """The synthetic regions (test_synthetic_regions_hit_their_shapes) under the
    default scoring, a = 2 scaling (b 8, gaps 12 + 2) and o_ins = 0: every field of
    every region equals the restatement; the regions next to an unmapped, bridging,
    empty or oversized one are untouched by it."""
    reads, regs, reg_off, tags = _synthetic(name == "default")
    want = _synthetic_ref(name)
    gpu = _gpu_for(_genome(), gpu_device)
    try:
        alns, cigar, md, ms = gpu.reg2aln(_pack(_genome()), G_LEN, reads.codes, reads.offs, regs, reg_off,
                                          _c_opt(OPTS[name]))
    finally:
        gpu.close()
    print(f"reg2aln synthetic {name}: {regs.size} regions, kernel {ms:.3f} ms")
    got = [_got(alns, cigar, md, k) for k in range(regs.size)]
    bad = [(tags[k], got[k], want[k]) for k in range(regs.size) if got[k] != want[k]]
    assert not bad, bad[:3]
    used = sum(int(a["n_cigar"]) for a in alns)
    assert used == cigar.size and sum(int(a["md_len"]) for a in alns) == md.size


@pytest.mark.gpu
def test_reg2aln_gpu_argument_checks(gpu_device):
    """The host API refuses a query code above 4, a short .pac and a missing
    resident .pac; a too-small pool gives SMEM_E_CAPACITY with the sizes needed,
    and the call repeated with them succeeds."""
    import smemgpu
    reads, regs, reg_off, _tags = _synthetic(True)
    want = _synthetic_ref("default")
    pac, opt = _pack(_genome()), _c_opt(ref.Opt())
    gpu = _gpu_for(_genome(), gpu_device)
    try:
        with pytest.raises(smemgpu.SmemError):   # no pac given, none resident
            gpu.reg2aln(None, G_LEN, reads.codes, reads.offs, regs, reg_off, opt)
        with pytest.raises(smemgpu.SmemError):   # short pac
            gpu.reg2aln(pac[:10], G_LEN, reads.codes, reads.offs, regs, reg_off, opt)
        bad = reads.codes.copy()
        bad[5] = 7
        with pytest.raises(smemgpu.SmemError):   # code > 4
            gpu.reg2aln(pac, G_LEN, bad, reads.offs, regs, reg_off, opt)
        need_c = sum(len(a.cigar) for a in want)
        need_m = sum(len(a.md) for a in want)
        lib = smemgpu.load()
        codes = np.ascontiguousarray(reads.codes, dtype=np.uint8)
        offs = np.ascontiguousarray(reads.offs, dtype=np.uint64)
        rg = np.ascontiguousarray(regs.astype(smemgpu.lib.ALNREG_DT))
        alns = np.zeros(regs.size, dtype=smemgpu.lib.ALN_DT)

        def call(cap_c, cap_m):
            cg, m = np.zeros(max(cap_c, 1), np.uint32), np.zeros(max(cap_m, 1), np.uint8)
            nc, nm = C.c_uint64(), C.c_uint64()
            rc = lib.smem_reg2aln(gpu._h, offs.size - 1, codes.ctypes.data, offs.ctypes.data, rg.ctypes.data,
                                  reg_off.ctypes.data, pac.ctypes.data, G_LEN, C.byref(opt), alns.ctypes.data,
                                  cg.ctypes.data, cap_c, C.byref(nc), m.ctypes.data, cap_m, C.byref(nm), None)
            return rc, int(nc.value), int(nm.value), cg, m
        rc, nc, nm, _, _ = call(3, need_m + 100)
        assert (rc, nc, nm) == (smemgpu.lib.SMEM_E_CAPACITY, need_c, need_m)
        rc, nc, nm, _, _ = call(need_c, need_m - 1)
        assert (rc, nc, nm) == (smemgpu.lib.SMEM_E_CAPACITY, need_c, need_m)
        rc, nc, nm, cg, m = call(need_c, need_m)
        assert (rc, nc, nm) == (0, need_c, need_m)
        assert all(_got(alns, cg, m, k) == want[k] for k in range(regs.size))
        # the binding repeats the call itself when its first guess is too small
        a2, c2, m2, _ = gpu.reg2aln(pac, G_LEN, reads.codes, reads.offs, regs, reg_off, opt, cigar_cap=1, md_cap=1)
        assert all(_got(a2, c2, m2, k) == want[k] for k in range(regs.size))
    finally:
        gpu.close()
