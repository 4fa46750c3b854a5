"""Loader for tests/golden/optaln/ (tests/golden/make_golden_optaln.py): the
reference's records of the r3 / r4 reads under nine option sets, beside the
reference's raw regions of the same reads and options that were committed with
the chains -> regions tests (tests/golden/<g>_<rs>_<oname>.smrg.gz).

Shared by tests/test_optaln.py (no GPU) and tests/test_gpu_optaln.py: every
restatement of a set is computed once per process and kept."""
import functools
import gzip
import hashlib
import json
import os

import numpy as np

import reg2aln_ref
import regfin_data
import regfin_ref
import xref_ref
from tests import aln_reads, golden_data

DIR = os.path.join(golden_data.GOLDEN, "optaln")
ONAMES = ("default", "gaps", "A3", "A100", "B1", "B9", "w1", "w7", "k10")
SETS = tuple(f"{g}_{rs}_{o}" for g, rs in (("g1", "r3"), ("g2", "r4")) for o in ONAMES)
MAX_UNMATCHED = 0.02


@functools.lru_cache(maxsize=None)
def manifest():
    with open(os.path.join(DIR, "manifest.json")) as fh:
        return json.load(fh)


def _sam_ops(s):
    import re
    return tuple(int(n) << 4 | (3 if op == "H" else "MIDS".index(op)) for n, op in re.findall(r"(\d+)([MIDSH])", s))


def _tag(s):
    return None if s == "." else int(s)


@functools.lru_cache(maxsize=None)
def load(name):
    """dict(g, oname, man, reads, regs, reg_off, lens, ids, l_pac, pac, contigs, records, hits, opt,
    aln_opt, fin_opt): regs / reg_off are the committed raw regions; ids[r] is read r's
    ordinal among the reads of at least 30 bp (the reference's hash id); records[r] lists the
    reference's mapped records of read r in print order as dicts with flag, rname, pos
    (1-based in the contig), mapq, cigar (SAM text), ops (smem_aln_t words), nm, md, AS, XS
    (None: tag absent), None for a read under 30 bp; hits[r][i] is the raw region with that
    record's geometry, or -1 (make_golden_cigar.match_records' rule); opt is the aln_reads
    dict, aln_opt / fin_opt the restatements' option objects (T = 30 a, as `bwa mem -A`)."""
    g, rs, oname = name.split("_", 2)
    man = manifest()[name]
    fix = next(f for f in golden_data.aln_fixtures() if f["file"] == name + ".smrg.gz")
    o = aln_reads.full_options(oname)
    assert man["opt"] == o == fix["opt"] and man["n_reads"] == fix["n_reads"]
    reads = golden_data.aln_reads(fix)
    regs, reg_off = golden_data.smrg_parse(golden_data.smrg(fix))
    lens = reads.lens.astype(np.int32)
    ids = np.cumsum(lens >= 30).astype(np.int64) - 1
    assert int((lens >= 30).sum()) == man["reads_kept"]
    with gzip.open(os.path.join(DIR, name + ".tsv.gz"), "rb") as fh:
        data = fh.read()
    assert hashlib.sha256(data).hexdigest() == man["sha256"], "fixture corrupted"
    l_pac = golden_data.l_pac(g)
    contigs = regfin_data.contigs(g)
    ctg_off = {c[0]: c[1] for c in contigs}
    records = [[] if lens[r] >= 30 else None for r in range(reads.n)]
    hits = [[] for _ in range(reads.n)]
    for line in data.decode().split("\n"):
        if not line:
            continue
        f = line.split("\t")
        r = int(f[0][1:])
        w = dict(flag=int(f[1]), rname=f[2], pos=int(f[3]), mapq=int(f[4]), cigar=f[5], ops=_sam_ops(f[5]),
                 nm=int(f[6]), md=f[7], AS=_tag(f[8]), XS=_tag(f[9]))
        records[r].append(w)
        # the region of the read with the record's strand, clips, position and reference length
        ops, rev, L = w["ops"], bool(w["flag"] & 16), int(lens[r])
        c5 = ops[0] >> 4 if ops[0] & 0xf == 3 else 0
        c3 = ops[-1] >> 4 if ops[-1] & 0xf == 3 and len(ops) > 1 else 0
        rlen = sum(c >> 4 for c in ops if c & 0xf in (0, 2))
        gpos, hit = ctg_off[w["rname"]] + w["pos"] - 1, -1
        for k in range(int(reg_off[r]), int(reg_off[r + 1])):
            rb, re_, qb, qe = (int(regs[k][x]) for x in ("rb", "re", "qb", "qe"))
            if rb < 0 or re_ < 0 or (rb < l_pac) == rev:
                continue
            if ((L - qe, qb) if rev else (qb, L - qe)) == (c5, c3) and (2 * l_pac - re_ if rev else rb) == gpos \
                    and re_ - rb == rlen:
                hit = k
                break
        hits[r].append(hit)
    so = {k: o[k] for k in ("a", "b", "o_del", "e_del", "o_ins", "e_ins")}
    return dict(g=g, oname=oname, man=man, reads=reads, regs=regs, reg_off=reg_off, lens=lens, ids=ids, l_pac=l_pac,
                pac=golden_data.pac(g), contigs=contigs, records=records, hits=hits, opt=o,
                aln_opt=reg2aln_ref.Opt(w=o["w"], **so),
                fin_opt=regfin_ref.Opt(min_seed_len=o["min_seed_len"], T=30 * o["a"], **so))


def record_tuple(F, w):
    """a reference record as reg2aln's (is_rev, pos on the forward strand, CIGAR words, NM, MD)"""
    off = next(c[1] for c in F["contigs"] if c[0] == w["rname"])
    return (int(bool(w["flag"] & 16)), off + w["pos"] - 1, w["ops"], w["nm"], w["md"])


# ------------------------------------------------------------------ restatements
_ALN = {}


def align(name, r, reg):
    """reg2aln_ref.reg2aln of one region of read r under the set's scoring; kept by the
    region's content, so a raw region and the final region made of it cost one DP"""
    F = load(name)
    key = (name, r) + tuple(int(reg[f]) for f in ("rb", "re", "qb", "qe", "truesc", "w"))
    if key not in _ALN:
        _ALN[key] = reg2aln_ref.reg2aln(F["aln_opt"], F["l_pac"], F["pac"], F["reads"].read(r), reg)
    return _ALN[key]


def read_of_region(reg_off):
    return np.repeat(np.arange(reg_off.size - 1), np.diff(reg_off.astype(np.int64)))


@functools.lru_cache(maxsize=None)
def raw_aligned(name):
    """the restatement's alignment of every raw region, in the file's order"""
    F = load(name)
    rd = read_of_region(F["reg_off"])
    return [align(name, int(rd[k]), F["regs"][k]) for k in range(F["regs"].size)]


@functools.lru_cache(maxsize=None)
def fin_rows(name):
    """regfin_ref.finalize per read: [(final regions, sel, selected indices)]"""
    F = load(name)
    return [regfin_ref.finalize(F["fin_opt"], F["regs"][int(F["reg_off"][r]):int(F["reg_off"][r + 1])], int(F["lens"][r]),
                                int(F["ids"][r])) for r in range(F["lens"].size)]


@functools.lru_cache(maxsize=None)
def fin_arrays(name):
    """the same as the arrays smem_reg_finalize returns (regfin_data.assert_equal's `want`)"""
    F = load(name)
    return regfin_data.restate(F["fin_opt"], F["regs"], F["reg_off"], F["lens"], F["ids"])


@functools.lru_cache(maxsize=None)
def expected(name):
    """what the resident chain's reg2aln gives: per read [(final region, Aln, rid)] in
    selection order (xref_ref.expected_rows over the two restatements)"""
    F = load(name)
    rows = xref_ref.aligned_rows(fin_rows(name), F["l_pac"], F["pac"], F["reads"], F["aln_opt"],
                                 align=lambda r, p: align(name, r, p))
    return xref_ref.expected_rows(rows, F["contigs"], F["l_pac"])


def shape_of(name, reg, aln):
    """reg2aln_ref.classify of an aligned region over the tries the restatement made"""
    return reg2aln_ref.classify(load(name)["aln_opt"], reg, max(aln.tries, 1))


def coverage(name, regs_alns):
    """what the (region, Aln) pairs reach in the GPU stage, by the restated classifier:
    dict(classes=[n per class], tries={tries: n}, deferred={class: n}, lds_retry_wide=n of
    retries run in a lane group's LDS with more columns than the group has lanes)"""
    out = dict(classes=[0, 0, 0, 0], tries={}, deferred={}, lds_retry_wide=0)
    for reg, aln in regs_alns:
        if aln.status != 0:
            continue
        s = shape_of(name, reg, aln)
        out["classes"][s.cls] += 1
        out["tries"][aln.tries] = out["tries"].get(aln.tries, 0) + 1
        if s.defer_try:
            out["deferred"][s.cls] = out["deferred"].get(s.cls, 0) + 1
        if s.cls < reg2aln_ref.SCRATCH_CLASS and any(n > s.group for n in s.n_col[1:s.in_lds_tries]):
            out["lds_retry_wide"] += 1
    return out
