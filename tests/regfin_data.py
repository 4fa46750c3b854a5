"""Fixtures shared by tests/test_regfin.py and tests/test_gpu_regfin.py: the
reference's raw regions (SMRG) beside the reference's own records, and the
restatement's prediction of those records."""
import functools
import gzip
import os
import struct

import numpy as np

import regfin_ref as ref
from tests import golden_data

SETS = ("g1_default_std", "g2_default_std", "cigar_g1", "cigar_g2", "g2_r4")


def contigs(g):
    """[(name, offset, length)] of the concatenated forward strand"""
    out, name, off, n = [], None, 0, 0
    for line in golden_data.gz(f"{g}.fa.gz").split(b"\n"):
        if line.startswith(b">"):
            if name is not None:
                out.append((name, off, n))
                off += n
            name, n = line[1:].split()[0].decode(), 0
        else:
            n += len(line.strip())
    out.append((name, off, n))
    return out


def _smrd(data):
    n = struct.unpack_from("<Q", data, 8)[0]
    return np.frombuffer(data, dtype="<i4", count=n, offset=24).astype(np.int32)


def _regfin_records(name, n_reads):
    """regfin/<name>.tsv.gz (tests/golden/make_golden_regfin.py) as per-read record lists"""
    import hashlib
    import json
    d = os.path.join(golden_data.GOLDEN, "regfin")
    with open(os.path.join(d, "manifest.json")) as fh:
        man = json.load(fh)[name]
    with gzip.open(os.path.join(d, name + ".tsv.gz"), "rb") as fh:
        data = fh.read()
    assert hashlib.sha256(data).hexdigest() == man["sha256"], "fixture corrupted"
    out = [[] for _ in range(n_reads)]
    for line in data.decode().split("\n"):
        if line:
            f = line.split("\t")
            out[int(f[0][1:])].append(dict(flag=int(f[1]), rname=f[2], pos=int(f[3]), mapq=int(f[4]),
                                           AS=None if f[5] == "." else int(f[5]),
                                           XS=None if f[6] == "." else int(f[6])))
    assert sum(len(r) for r in out) == man["records"]
    return out


@functools.lru_cache(maxsize=None)
def load(name):
    """dict(g, regs, reg_off, lens, ids, l_pac, records): records[r] is the list of the
    reference's mapped records of read r, in print order, as dicts with flag, rname,
    pos (1-based, in the contig), mapq, AS, XS (None when the tag is absent); None for a
    read the reference never saw (under 30 bp).  g*_default_std: the single-end golden SAM;
    cigar_g*: the gapped reads' records (cigar/<g>.tsv.gz, with MAPQ, AS and XS from
    regfin/cigar_<g>.tsv.gz); g2_r4: the r4 reads' regions and regfin/g2_r4.tsv.gz"""
    if name.startswith("cigar_"):
        g = name[6:]
        d = os.path.join(golden_data.GOLDEN, "cigar")
        with gzip.open(os.path.join(d, f"{g}.smrd.gz"), "rb") as fh:
            lens = _smrd(fh.read())
        with gzip.open(os.path.join(d, f"{g}.smrg.gz"), "rb") as fh:
            regs, reg_off = golden_data.smrg_parse(fh.read())
        records = [[] for _ in range(lens.size)]
        with gzip.open(os.path.join(d, f"{g}.tsv.gz"), "rt") as fh:
            for line in fh:
                f = line.rstrip("\n").split("\t")
                records[int(f[0][1:])].append(dict(flag=int(f[1]), rname=f[2], pos=int(f[3]), cigar=f[4],
                                                   nm=int(f[5]), md=f[6]))
        ids = np.arange(lens.size, dtype=np.int64)
        more = _regfin_records(name, lens.size)
        for r, recs in enumerate(records):
            assert [(w["flag"], w["rname"], w["pos"]) for w in recs] == \
                [(w["flag"], w["rname"], w["pos"]) for w in more[r]], "the two record files disagree"
            for w, m in zip(recs, more[r]):
                w.update(mapq=m["mapq"], AS=m["AS"], XS=m["XS"])
    elif name == "g2_r4":
        g = "g2"
        fix = next(f for f in golden_data.aln_fixtures() if f["file"] == "g2_r4_default.smrg.gz")
        regs, reg_off = golden_data.smrg_parse(golden_data.smrg(fix))
        lens = golden_data.aln_reads(fix).lens.astype(np.int32)
        ids = np.cumsum(lens >= 30).astype(np.int64) - 1
        records = _regfin_records(name, lens.size)
        records = [recs if lens[r] >= 30 else None for r, recs in enumerate(records)]
    else:
        g = name[:2]
        fix = next(f for f in golden_data.aln_fixtures() if f["file"] == name + ".smrg.gz")
        regs, reg_off = golden_data.smrg_parse(golden_data.smrg(fix))
        n = reg_off.size - 1
        with gzip.open(os.path.join(golden_data.GOLDEN, "r1.smrd.gz" if g == "g1" else "r2.smrd.gz"), "rb") as fh:
            lens = _smrd(fh.read())[:n]
        # the reference numbers the reads of its FASTQ, which omits reads under 30 bp
        ids = np.cumsum(lens >= 30).astype(np.int64) - 1
        records = [[] if lens[r] >= 30 else None for r in range(n)]
        with gzip.open(os.path.join(golden_data.GOLDEN, "sam", f"{g}_se.sam.gz"), "rt") as fh:
            for line in fh:
                if line.startswith("@"):
                    continue
                f = line.rstrip("\n").split("\t")
                flag = int(f[1])
                r = int(f[0][1:])
                assert records[r] is not None
                if flag & 4:
                    continue
                tags = {t[:2]: int(t[5:]) for t in f[11:] if t[:5] in ("AS:i:", "XS:i:")}
                records[r].append(dict(flag=flag, rname=f[2], pos=int(f[3]), mapq=int(f[4]), cigar=f[5],
                                       AS=tags.get("AS"), XS=tags.get("XS")))
    return dict(g=g, regs=regs, reg_off=reg_off, lens=lens, ids=ids, l_pac=golden_data.l_pac(g), records=records,
                contigs=contigs(g))


def predict_records(F, r, a, sel, idx):
    """what the reference prints for read r, from the stage's output (a: final regions
    as records with rb / re / score, sel[k] = (mapq, flag, xs), idx: selected regions):
    a list of dicts like load()'s records; pos / rname None for a region that bridges a
    contig boundary (bwa_fix_xref2 moves it: the caller's business)"""
    out = []
    l_pac = F["l_pac"]
    for k in idx:
        p = a[k]
        mapq, flag, xs = (int(v) for v in sel[k])
        rb, re_ = int(p["rb"]), int(p["re"])
        rev = rb >= l_pac
        fb, fe = (2 * l_pac - re_, 2 * l_pac - rb) if rev else (rb, re_)
        rname = pos = None
        for cname, off, n in F["contigs"]:
            if off <= fb and fe <= off + n:
                rname, pos = cname, fb - off + 1
        out.append(dict(flag=flag | (16 if rev else 0), rname=rname, pos=pos, mapq=mapq, AS=int(p["score"]),
                        XS=xs if xs >= 0 else None))
    return out


@functools.lru_cache(maxsize=None)
def restated(name, **kw):
    """finalize() over every read of a set: (list of (a, sel, idx) per read, Counters)"""
    F = load(name)
    ctr = ref.Counters()
    opt = ref.Opt(**kw)
    out = []
    for r in range(F["lens"].size):
        lo, hi = int(F["reg_off"][r]), int(F["reg_off"][r + 1])
        out.append(ref.finalize(opt, F["regs"][lo:hi], int(F["lens"][r]), int(F["ids"][r]), ctr))
    return out, ctr


# ------------------------------------------------------------ synthetic reads
def _alnreg():
    from smemgpu.lib import ALNREG_DT
    return ALNREG_DT


def synth_regions(rng, n, span=60, qspan=60, max_len=40, scores=(25, 45), sorted_re=False):
    """n random regions drawn from a small coordinate range, so that equal keys,
    overlaps, redundant pairs and identical hits are dense"""
    a = np.zeros(n, dtype=_alnreg())
    a["rb"] = 5000 + rng.integers(0, span, n)
    a["re"] = a["rb"] + rng.integers(1, max_len, n)
    a["qb"] = rng.integers(0, qspan, n)
    a["qe"] = a["qb"] + rng.integers(1, max_len, n)
    a["score"] = rng.integers(scores[0], scores[1], n)
    a["truesc"] = a["score"]
    a["csub"] = np.where(rng.random(n) < 0.3, rng.integers(0, scores[1], n), 0)
    a["sub_n"] = np.where(rng.random(n) < 0.1, rng.integers(1, 5, n), 0)
    a["w"] = 100
    a["seedcov"] = rng.integers(1, 60, n)
    if sorted_re:   # ascending input with equal keys uses up the introsort's depth budget
        a = a[np.argsort(a["re"], kind="stable")]
    return a


SYNTH_SIZES = (0, 1, 2, 3, 15, 16, 17, 18, 33, 34, 35, 63, 64, 65, 129)


def synth_reads(seed=7, extra=()):
    """(regs, reg_off, read_len): reads of SYNTH_SIZES regions (twice, with other draws),
    one of 300 regions in ascending re with equal keys (reaches the combsort), one of
    equal scores spread out (a long second and third sort), and `extra` arrays"""
    rng = np.random.default_rng(seed)
    parts = [synth_regions(rng, n) for n in SYNTH_SIZES]
    parts += [synth_regions(rng, n, span=400, qspan=100, max_len=25) for n in SYNTH_SIZES]
    parts.append(synth_regions(rng, 300, span=200, qspan=100, sorted_re=True))
    parts.append(synth_regions(rng, 200, span=4000, qspan=100, max_len=20, scores=(30, 32)))
    parts += list(extra)
    reg_off = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)
    return np.concatenate(parts), reg_off, np.full(len(parts), 100, dtype=np.int32)


def restate(opt, regs, reg_off, read_len, ids, ctr=None):
    """finalize() per read -> the arrays the stage returns (regs ALNREG_DT, out_off, sel rows,
    sel_idx as indices into regs, sel_off, status)"""
    out, sel, sidx, out_off, sel_off, status = [], [], [], [0], [0], []
    for r in range(read_len.size):
        lo, hi = int(reg_off[r]), int(reg_off[r + 1])
        if hi - lo > ref.MAX_REGS:
            a, s, idx = [], [], []
            status.append(1)
        else:
            a, s, idx = ref.finalize(opt, regs[lo:hi], int(read_len[r]), int(ids[r]), ctr)
            status.append(0)
        sidx += [out_off[-1] + k for k in idx]
        out += [tuple(p[f] for f in ref.FIELDS) for p in a]
        sel += s
        out_off.append(out_off[-1] + len(a))
        sel_off.append(sel_off[-1] + len(idx))
    return dict(regs=np.array(out, dtype=_alnreg()) if out else np.zeros(0, dtype=_alnreg()),
                out_off=np.array(out_off, dtype=np.uint64), sel=np.array(sel, dtype=np.int32).reshape(-1, 3),
                sel_idx=np.array(sidx, dtype=np.uint64), sel_off=np.array(sel_off, dtype=np.uint64),
                status=np.array(status, dtype=np.int32))


def assert_equal(got, want):
    """every field of every output of the stage (got: smemgpu FinResults) equals the restatement"""
    assert np.array_equal(got.status, want["status"])
    assert np.array_equal(got.out_off, want["out_off"]), "out_off"
    assert np.array_equal(got.sel_off, want["sel_off"]), "sel_off"
    for f in ref.FIELDS:
        bad = np.nonzero(got.regs[f] != want["regs"][f])[0]
        assert bad.size == 0, (f, int(bad[0]), got.regs[bad[0]], want["regs"][bad[0]])
    g = np.stack([got.sel["mapq"], got.sel["flag"], got.sel["xs"]], axis=1).reshape(-1, 3)
    bad = np.nonzero((g != want["sel"]).any(axis=1))[0]
    assert bad.size == 0, (int(bad[0]), g[bad[0]], want["sel"][bad[0]])
    assert np.array_equal(got.sel_idx, want["sel_idx"]), "sel_idx"
