"""Regenerate the committed golden fixtures from the compiled reference.

    python tests/golden/make_golden.py

Needs oracle/_ref/ref_harness (built by `make -C oracle ref`, which compiles
the reference's own C sources in place from /root/reference/software).
Inputs are seeded synthetic data; every output file here is produced by the
reference code itself:

  g1.fa.gz            genome (300 kbp, 4 records, repeat families / exact / tandem repeats)
  g1.bwt.gz           `bwa index -a is` of g1.fa   (software/bwtindex.c:187)
  r1.smrd.gz          1500 reads (SMRD, include/smem_formats.h), mixed shapes
  g1_<case>.smgo.gz   reference smem_next2 streams under mem_insert_seed
                      (software/bwamem.c:453-460) for each option set
  g1.sa.gz            the `bwa index` sampled suffix array (.sa, software/bwt.c:852)
  g1_<case>.smsa.gz   reference bwt_sa() of every seed occurrence of that stream
                      (software/bwamem.c:467-474, max_occ 10000)
  g1_<case>_<chain>_f<0|1>.smch.gz
                      reference mem_chain() of every read (software/bwamem.c:593),
                      without (f0) and with (f1) mem_chain_flt() (software/bwamem.c:629)
  manifest.json       cases, options, sha256 of the uncompressed streams

  g2.*, g2_<case>*     the same for a repeat-dense genome (make_g2)
  ksw.smkt.gz         5000 SW extension problems (include/smem_formats.h) shaped like
                      mem_chain2aln's left/right extensions on g1 (software/bwamem.c:1120-1170)
  ksw.smkr.gz         the reference's own ksw_extend2 on each (software/ksw.c:379)
  ksw_gap0.smk[tr].gz 500 more with both gap opens 0, and the reference's results

    python tests/golden/make_golden.py --chains-only   # (re)make only the g1 .smch files
    python tests/golden/make_golden.py --g2-only       # (re)make only the g2 set
    python tests/golden/make_golden.py --ksw-only      # (re)make only the ksw set
    python tests/golden/make_golden.py --ksw-gap0-only # (re)make only ksw_gap0
    python tests/golden/make_golden.py --kswa-only     # (re)make only the ksw_align2 sets
    python tests/golden/make_golden.py --aln-only      # (re)make the region fixtures (*.smrg.gz, r3 / r4 and theirs)
    python tests/golden/make_golden.py --aln-options-only  # (re)make only r3 / r4 and their fixtures
    python tests/golden/make_golden.py --long-only     # (re)make only long/ (on the committed g1 .bwt / .sa)
  long/r5.smrd.gz     16 reads of 321 bp to 70 kbp on g1 (tests/long_reads.py class_reads)
  long/g1_r5_default.smgo.gz, .smsa.gz, _std_f<0|1>.smch.gz
                      the reference's lists, bwt_sa positions (max_occ 10000) and chains of them
                      under the default options; long/manifest.json
  r3.smrd.gz, r4.smrd.gz  reads of g1 / g2 with indels, junk stretches, mismatched ends and unrelated
                      tails (tests/aln_reads.py), their filtered chains <g>_<r>_<std|k10|w1|w7>_std_f1.smch.gz
  <g>_<r>_<set>.smrg.gz  the reference's regions of those reads under each option set of
                      aln_reads.OPTION_SETS (`ref_harness aln` with the scoring arguments)
  kswa_a<1|2>.smat.gz 3000 ksw_align2 problems shaped like mem_chain2aln_short's (a = 1, 2)
  kswa_a<1|2>.smar.gz the reference's own ksw_align2 on each (software/ksw.c:342)
  kswa_<set>.sma[tr].gz  up to 600 each (KSWA_MORE): o_ins = 0 at a = 1 and 2, asymmetric gaps,
                      o_del = 0, KSW_XSTOP, 200-256 bp queries, the length edges and the
                      longest suboptimal list, byte saturation at a = 2 and a = 1
"""
import gzip
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem-harp2_amd"))
sys.path.insert(0, ROOT)

from smemgpu import synth  # noqa: E402
from oracle import oracle  # noqa: E402

MAX_OCC = 10000  # mem_opt_t.max_occ default of this reference (software/bwamem.c:60)

CASES = [
    dict(name="default", n_reads=1500, opt=dict(min_seed_len=19, split_factor=1.5, split_width=10, start_width=1)),
    dict(name="noexact", n_reads=500, opt=dict(min_seed_len=19, split_factor=1.5, split_width=10, start_width=2)),
    dict(name="k14s20", n_reads=500, opt=dict(min_seed_len=14, split_factor=1.5, split_width=20, start_width=1)),
    dict(name="reseed", n_reads=500, opt=dict(min_seed_len=19, split_factor=1.0, split_width=500, start_width=1)),
    dict(name="k30", n_reads=500, opt=dict(min_seed_len=30, split_factor=2.0, split_width=3, start_width=1)),
]


# chain option sets (mem_opt_t w / max_chain_gap / mask_level / chain_drop_ratio,
# software/bwamem.c:53-64); "std" is mem_opt_init's
CHAIN_OPTS = [
    dict(name="std", w=100, max_chain_gap=10000, mask_level=0.5, drop_ratio=0.5),
    dict(name="tight", w=5, max_chain_gap=40, mask_level=0.3, drop_ratio=0.8),
]
CHAIN_CASES = {"default": ["std", "tight"], "noexact": ["std"], "k14s20": ["std", "tight"], "reseed": ["std"],
               "k30": ["std"]}


def ref_chain(tmp, smrd, case, copt, filt, genome="g1"):
    out = os.path.join(tmp, "c.smch")
    o = case["opt"]
    subprocess.run([oracle.REF, "chain", os.path.join(tmp, genome + ".bwt"), os.path.join(tmp, genome + ".sa"), smrd,
                    out,
                    str(o["min_seed_len"]), str(o["split_factor"]), str(o["split_width"]), str(o["start_width"]),
                    str(MAX_OCC), str(copt["w"]), str(copt["max_chain_gap"]), str(copt["mask_level"]),
                    str(copt["drop_ratio"]), str(filt)], check=True)
    with open(out, "rb") as fh:
        return fh.read()


def make_chains(tmp, reads, manifest):
    """chain fixtures for every case of the manifest (files g1.bwt / g1.sa in tmp)"""
    copts = {c["name"]: c for c in CHAIN_OPTS}
    for case in manifest["cases"]:
        sub = reads.subset(np.arange(case["n_reads"]))
        p = os.path.join(tmp, "sub.smrd")
        synth.write_smrd(p, sub)
        case["chains"] = []
        for cname in CHAIN_CASES[case["name"]]:
            for filt in (0, 1):
                data = ref_chain(tmp, p, case, copts[cname], filt)
                fn = f"g1_{case['name']}_{cname}_f{filt}.smch.gz"
                gz_write(os.path.join(HERE, fn), data)
                case["chains"].append(dict(copts[cname], file=fn, filter=filt,
                                           sha256=hashlib.sha256(data).hexdigest()))


G2_CASES = [
    dict(name="default", opt=dict(min_seed_len=19, split_factor=1.5, split_width=10, start_width=1)),
    dict(name="k14s20", opt=dict(min_seed_len=14, split_factor=1.5, split_width=20, start_width=1)),
]


def make_g2():
    """g2: a repeat-dense genome (60 % copies of 4 families, tandem and exact
    repeats) whose reads carry tens to hundreds of seeds and chains, so the
    chain tree splits to several levels and the chain filter sorts long
    lists.  Files g2.* and manifest["g2"]."""
    if not oracle.ref_available():
        oracle.build(ref=True)
    tmp = tempfile.mkdtemp()
    try:
        genome = synth.make_genome(150_000, seed=21, repeat_frac=0.6, n_families=4, exact_frac=0.01,
                                   tandem_frac=0.01)
        fa = os.path.join(tmp, "g2.fa")
        synth.write_fasta(fa, genome)
        oracle.ref_index(fa, os.path.join(tmp, "g2"))
        reads = synth.concat_reads([synth.make_reads(genome.codes, 300, 150, seed=201),
                                    synth.make_reads(genome.codes, 100, 250, seed=202, sub_rate=0.01),
                                    synth.make_reads(genome.codes, 100, (15, 200), seed=203, n_rate=0.01)])
        smrd = os.path.join(tmp, "r2.smrd")
        synth.write_smrd(smrd, reads)
        for src, dst in (("g2.fa", "g2.fa.gz"), ("g2.bwt", "g2.bwt.gz"), ("g2.sa", "g2.sa.gz"),
                         ("r2.smrd", "r2.smrd.gz")):
            with open(os.path.join(tmp, src), "rb") as fh:
                gz_write(os.path.join(HERE, dst), fh.read())
        cases = []
        copts = {c["name"]: c for c in CHAIN_OPTS}
        for case in G2_CASES:
            out = os.path.join(tmp, case["name"] + ".smgo")
            oracle.ref_smem(os.path.join(tmp, "g2.bwt"), smrd, out, **case["opt"])
            with open(out, "rb") as fh:
                data = fh.read()
            gz_write(os.path.join(HERE, f"g2_{case['name']}.smgo.gz"), data)
            sa_out = os.path.join(tmp, case["name"] + ".smsa")
            oracle.ref_sa(os.path.join(tmp, "g2.bwt"), os.path.join(tmp, "g2.sa"), out, sa_out,
                          min_seed_len=case["opt"]["min_seed_len"], max_occ=MAX_OCC)
            with open(sa_out, "rb") as fh:
                sa_data = fh.read()
            gz_write(os.path.join(HERE, f"g2_{case['name']}.smsa.gz"), sa_data)
            c = dict(case, n_reads=reads.n, sha256=hashlib.sha256(data).hexdigest(), max_occ=MAX_OCC,
                     sa_sha256=hashlib.sha256(sa_data).hexdigest(), chains=[])
            for cname in ("std", "tight"):
                for filt in (0, 1):
                    cd = ref_chain(tmp, smrd, case, copts[cname], filt, genome="g2")
                    fn = f"g2_{case['name']}_{cname}_f{filt}.smch.gz"
                    gz_write(os.path.join(HERE, fn), cd)
                    c["chains"].append(dict(copts[cname], file=fn, filter=filt,
                                            sha256=hashlib.sha256(cd).hexdigest()))
            cases.append(c)
        with open(os.path.join(HERE, "manifest.json")) as fh:
            manifest = json.load(fh)
        manifest["g2"] = {"genome": dict(n_bp=150_000, seed=21, repeat_frac=0.6, n_families=4), "cases": cases}
        with open(os.path.join(HERE, "manifest.json"), "w") as fh:
            json.dump(manifest, fh, indent=1)
    finally:
        shutil.rmtree(tmp)


def chains_only():
    if not oracle.ref_available():
        oracle.build(ref=True)
    tmp = tempfile.mkdtemp()
    try:
        for name in ("g1.bwt", "g1.sa"):
            with gzip.open(os.path.join(HERE, name + ".gz"), "rb") as fh, open(os.path.join(tmp, name), "wb") as o:
                o.write(fh.read())
        with gzip.open(os.path.join(HERE, "r1.smrd.gz"), "rb") as fh, open(os.path.join(tmp, "r1.smrd"), "wb") as o:
            o.write(fh.read())
        reads = synth.read_smrd(os.path.join(tmp, "r1.smrd"))
        with open(os.path.join(HERE, "manifest.json")) as fh:
            manifest = json.load(fh)
        make_chains(tmp, reads, manifest)
        with open(os.path.join(HERE, "manifest.json"), "w") as fh:
            json.dump(manifest, fh, indent=1)
    finally:
        shutil.rmtree(tmp)


def make_reads(g):
    parts = [
        synth.make_reads(g, 500, 150, seed=101),
        synth.make_reads(g, 200, 100, seed=102),
        synth.make_reads(g, 200, 250, seed=103),
        synth.make_reads(g, 200, 150, seed=104, sub_rate=0.05),
        synth.make_reads(g, 200, (1, 320), seed=105, n_rate=0.02),
        synth.make_reads(g, 100, 101, seed=106, random_frac=1.0),
        synth.make_reads(g, 100, (10, 40), seed=107),
    ]
    r = synth.concat_reads(parts)
    perm = np.random.default_rng(108).permutation(r.n)
    return r.subset(perm)


def gz_write(path, data: bytes):
    with gzip.GzipFile(path, "wb", mtime=0) as fh:
        fh.write(data)


def main():
    if not oracle.ref_available():
        oracle.build(ref=True)
    tmp = tempfile.mkdtemp()
    try:
        genome = synth.make_genome(300_000, seed=11)
        fa = os.path.join(tmp, "g1.fa")
        synth.write_fasta(fa, genome)
        oracle.ref_index(fa, os.path.join(tmp, "g1"))
        reads = make_reads(genome.codes)
        smrd = os.path.join(tmp, "r1.smrd")
        synth.write_smrd(smrd, reads)
        with open(fa, "rb") as fh:
            gz_write(os.path.join(HERE, "g1.fa.gz"), fh.read())
        with open(os.path.join(tmp, "g1.bwt"), "rb") as fh:
            gz_write(os.path.join(HERE, "g1.bwt.gz"), fh.read())
        with open(os.path.join(tmp, "g1.sa"), "rb") as fh:
            gz_write(os.path.join(HERE, "g1.sa.gz"), fh.read())
        with open(smrd, "rb") as fh:
            gz_write(os.path.join(HERE, "r1.smrd.gz"), fh.read())
        manifest = {"genome": dict(n_bp=300_000, seed=11), "cases": []}
        for case in CASES:
            sub = reads.subset(np.arange(case["n_reads"]))
            p = os.path.join(tmp, "sub.smrd")
            synth.write_smrd(p, sub)
            out = os.path.join(tmp, case["name"] + ".smgo")
            oracle.ref_smem(os.path.join(tmp, "g1.bwt"), p, out, **case["opt"])
            with open(out, "rb") as fh:
                data = fh.read()
            gz_write(os.path.join(HERE, f"g1_{case['name']}.smgo.gz"), data)
            parsed = synth.read_smgo(data)
            sa_out = os.path.join(tmp, case["name"] + ".smsa")
            oracle.ref_sa(os.path.join(tmp, "g1.bwt"), os.path.join(tmp, "g1.sa"), out, sa_out,
                          min_seed_len=case["opt"]["min_seed_len"], max_occ=MAX_OCC)
            with open(sa_out, "rb") as fh:
                sa_data = fh.read()
            gz_write(os.path.join(HERE, f"g1_{case['name']}.smsa.gz"), sa_data)
            manifest["cases"].append(dict(case, sha256=hashlib.sha256(data).hexdigest(),
                                          n_intv=int(sum(a.shape[0] for r in parsed for a in r)),
                                          n_calls=int(sum(len(r) for r in parsed)),
                                          max_occ=MAX_OCC, sa_sha256=hashlib.sha256(sa_data).hexdigest(),
                                          n_occ=int(sum(p.size for p in synth.read_smsa(sa_data)))))
        make_chains(tmp, reads, manifest)
        with open(os.path.join(HERE, "manifest.json"), "w") as fh:
            json.dump(manifest, fh, indent=1)
        print(json.dumps(manifest, indent=1))
    finally:
        shutil.rmtree(tmp)


def make_ksw():
    if not oracle.ref_available():
        oracle.build(ref=True)
    tmp = tempfile.mkdtemp()
    try:
        with gzip.open(os.path.join(HERE, "g1.fa.gz"), "rb") as fh:
            from tests import golden_data
            g = golden_data.fasta_codes(fh.read())
        b = synth.make_ksw_tasks(g, 5000, seed=121)
        p = os.path.join(tmp, "ksw.smkt")
        synth.write_smkt(p, b)
        oracle.ref_ksw(p, os.path.join(tmp, "ksw.smkr"))
        for name in ("ksw.smkt", "ksw.smkr"):
            with open(os.path.join(tmp, name), "rb") as fh:
                gz_write(os.path.join(HERE, name + ".gz"), fh.read())
    finally:
        shutil.rmtree(tmp)
    make_ksw_gap0()


def make_ksw_gap0():
    """ksw_gap0.smkt/.smkr: 500 extension problems with both gap opens 0 (e = 1)"""
    if not oracle.ref_available():
        oracle.build(ref=True)
    tmp = tempfile.mkdtemp()
    try:
        with gzip.open(os.path.join(HERE, "g1.fa.gz"), "rb") as fh:
            from tests import golden_data
            g = golden_data.fasta_codes(fh.read())
        b = synth.make_ksw_tasks(g, 500, seed=122)
        b.o_del = b.o_ins = 0
        p = os.path.join(tmp, "ksw_gap0.smkt")
        synth.write_smkt(p, b)
        oracle.ref_ksw(p, os.path.join(tmp, "ksw_gap0.smkr"))
        for name in ("ksw_gap0.smkt", "ksw_gap0.smkr"):
            with open(os.path.join(tmp, name), "rb") as fh:
                gz_write(os.path.join(HERE, name + ".gz"), fh.read())
    finally:
        shutil.rmtree(tmp)


# ksw_align2 (software/ksw.c:342), the DP of mem_chain2aln_short: mem_opt_init's
# scoring (a 1, b 4, gaps 6 + 1: byte problems) and -A 2 scaled (a 2, b 8,
# gaps 12 + 2: queries of 125 bp and more take ksw_i16)
KSWA_SETS = [("kswa_a1", 1, 4, 6, 1, 151), ("kswa_a2", 2, 8, 12, 2, 152)]


X_BYTE, X_STOP, X_SUBO, X_START = synth.KSW_XBYTE, synth.KSW_XSTOP, synth.KSW_XSUBO, synth.KSW_XSTART


def _kswa_batch(items, a, b, o_del, e_del, o_ins, e_ins):
    """KswBatch of (query, target, xtra) items under one scoring"""
    tasks = np.zeros(len(items), dtype=synth.KSWA_TASK)
    qo = to = 0
    for k, (q, t, xtra) in enumerate(items):
        tasks[k] = (qo, to, q.size, t.size, xtra, 0)
        qo += q.size
        to += t.size
    cat = lambda xs: np.concatenate([np.asarray(x, dtype=np.uint8) for x in xs]) if xs else np.zeros(0, np.uint8)
    return synth.KswBatch(tasks, cat([i[0] for i in items]), cat([i[1] for i in items]), synth.bwa_scmat(a, b),
                          o_del, e_del, o_ins, e_ins)


def _short_pair(G, rng, qlo, qhi, sub, indel, n_runs=0, fit=False, exact=False):
    """One mem_chain2aln_short-shaped pair: a read of qlo..qhi bp copied from the
    genome with substitutions and indels (synth._mutated_copy), n_runs extra
    runs of 2..6 inserted bases (an insertion that crosses a block of the
    striped query is what the lazy-F loop carries), against the reference
    span padded and shifted by up to 50 (fit: never cut short of the read's
    end while 256 bp hold it; exact: the mutated read is of the drawn length
    itself); 30 % on the reverse strand"""
    ql = int(rng.integers(qlo, qhi + 1))
    pos = int(rng.integers(300, G.size - ql - 300))
    read = synth._mutated_copy(G[pos:pos + ql + (40 if exact else 0)], rng, sub, indel)
    if exact:
        read = read[:ql]
        assert read.size == ql
    for _ in range(n_runs):
        at = int(rng.integers(1, max(2, read.size)))
        read = np.concatenate([read[:at], rng.integers(0, 4, size=int(rng.integers(2, 7))).astype(np.uint8), read[at:]])
    read = read[:qhi]
    if read.size == 0:
        read = G[pos:pos + 1].copy()
    lo = pos - int(rng.integers(0, min(40, 257 - ql) if fit else 40))
    t = G[lo:lo + max(1, min(256, ql + int(rng.integers(0 if fit else -50, 51)) + (pos - lo)))].copy()
    if rng.random() < 0.3:
        read = (3 - read)[::-1].astype(np.uint8)
        t = (3 - t)[::-1].astype(np.uint8)
    return read.astype(np.uint8), t.astype(np.uint8)


def _short_xtra(qlen, a, min_seed_len=19):
    """mem_chain2aln_short's flags (software/bwamem.c:835)"""
    return X_SUBO | X_START | (X_BYTE if qlen * a < 250 else 0) | (min_seed_len * a)


def kswa_oins0(G, seed, a):
    """o_ins = 0 (bwa mem -O o,0): the lazy-F loop ends at its first step, so F
    crosses a block boundary into one column only.  Reads with 4 % indels and
    two longer insertions each."""
    rng = np.random.default_rng(seed)
    items = []
    for _ in range(600):
        q, t = _short_pair(G, rng, 60, 199, float(rng.choice([0.0, 0.01, 0.03])), 0.04, n_runs=2)
        items.append((q, t, _short_xtra(q.size, a)))
    return _kswa_batch(items, a, 4 * a, 6 * a, a, 0, a)


def kswa_xstop(G, seed):
    """KSW_XSTOP | v in the caller's xtra: the forward pass ends at the first
    row whose maximum reaches v.  v in {20, 40, 100} with and without XSUBO
    (v is then the suboptimal threshold too) and XSTART, byte and 16-bit."""
    rng = np.random.default_rng(seed)
    items = []
    for k in range(600):
        q, t = _short_pair(G, rng, 60, 199, float(rng.choice([0.0, 0.01, 0.03])), float(rng.choice([0.0, 0.01])))
        xtra = X_STOP | (20, 40, 100)[k % 3] | (X_SUBO if k // 3 % 2 else 0) | (X_START if k // 6 % 2 else 0) | \
            (X_BYTE if k // 12 % 2 else 0)
        items.append((q, t, xtra))
    return _kswa_batch(items, 1, 4, 6, 1, 6, 1)


def kswa_long(G, seed):
    """queries of 200..256 bp (the fourth 64-column chunk of the wave), 16-bit"""
    rng = np.random.default_rng(seed)
    items = []
    for _ in range(500):
        q, t = _short_pair(G, rng, 200, 256, float(rng.choice([0.0, 0.01, 0.03, 0.06])),
                           float(rng.choice([0.0, 0.005, 0.02])), fit=rng.random() < 0.5, exact=True)
        if rng.random() < 0.15:
            q[rng.random(q.size) < 0.02] = 4
        items.append((q, t, X_SUBO | X_START | 19))
    return _kswa_batch(items, 1, 4, 6, 1, 6, 1)


EDGE_QLEN = [1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256]
EDGE_TLEN = [0, 1, 63, 64, 65, 255, 256]


def kswa_edge(seed, byte):
    """every query length around a multiple of the vector width (8 and 16) and
    of the wave's 64-column chunk against every target length around the
    chunk, as a matching, a 10 %-mutated and an all-N query; the byte set adds
    the longest suboptimal list: `A` (and `AC`) against (AC)^128 with a
    threshold of 1 lists every second row, 128 entries"""
    rng = np.random.default_rng(seed)
    items = []
    for qlen in EDGE_QLEN:
        for tlen in EDGE_TLEN:
            for kind in range(3):
                q = rng.integers(0, 4, size=qlen).astype(np.uint8)
                if tlen >= qlen:
                    off = int(rng.integers(0, tlen - qlen + 1))
                    t = np.concatenate([rng.integers(0, 4, size=off), q, rng.integers(0, 4, size=tlen - qlen - off)])
                else:
                    off = int(rng.integers(0, qlen - tlen + 1))
                    t = q[off:off + tlen].copy()
                if kind == 1:
                    m = synth._mutated_copy(q, rng, 0.08, 0.02)
                    q = np.concatenate([m, rng.integers(0, 4, size=qlen)]).astype(np.uint8)[:qlen]
                elif kind == 2:
                    q[:] = 4
                items.append((q, t.astype(np.uint8), X_SUBO | X_START | (X_BYTE if byte else 0) | 19))
    if byte:
        ac = np.tile(np.array([0, 1], np.uint8), 128)
        items.append((ac[:1].copy(), ac, X_SUBO | X_START | X_BYTE | 1))
        items.append((ac[:2].copy(), ac, X_SUBO | X_START | X_BYTE | 1))
    return _kswa_batch(items, 1, 4, 6, 1, 6, 1)


def kswa_sat(G, seed, a):
    """byte scores at the ceiling: ksw_u8 stops at gmax + shift >= 255 and
    returns score 255, qe -1.  Clean and lightly mutated reads whose full match
    scores 220..256: at a = 2 (bias 8) 110..124 bp, at a = 1 (bias 4) 245..256
    bp with KSW_XBYTE forced"""
    rng = np.random.default_rng(seed)
    lo, hi = (110, 124) if a == 2 else (245, 256)
    items = []
    for k in range(400):
        ql = int(rng.integers(lo, hi + 1)) if k % 2 else int(rng.integers(hi - 2, hi + 1))
        sub = float(rng.choice([0.0, 0.0, 0.0, 0.01]))
        q, t = _short_pair(G, rng, ql, ql, sub, 0.0, fit=True)
        items.append((q, t[:256], X_SUBO | X_START | X_BYTE | 19 * a))
    return _kswa_batch(items, a, 4 * a, 6 * a, a, 6 * a, a)


def kswa_gaps(G, seed, o_del, e_del, o_ins, e_ins):
    """the make_kswa_tasks mix under other gap penalties"""
    kb = synth.make_kswa_tasks(G, 300, seed=seed)
    kb.o_del, kb.e_del, kb.o_ins, kb.e_ins = o_del, e_del, o_ins, e_ins
    return kb


# the sets that go past kswa_a1 / kswa_a2: o_ins = 0, asymmetric gaps and
# o_del = 0, KSW_XSTOP, 200-256 bp, the length edges, byte saturation
KSWA_MORE = [
    ("kswa_oins0", lambda G: kswa_oins0(G, 161, 1)),
    ("kswa_oins0_a2", lambda G: kswa_oins0(G, 162, 2)),
    ("kswa_asym", lambda G: kswa_gaps(G, 163, 5, 3, 8, 1)),
    ("kswa_odel0", lambda G: kswa_gaps(G, 164, 0, 2, 8, 1)),
    ("kswa_xstop", lambda G: kswa_xstop(G, 165)),
    ("kswa_long", lambda G: kswa_long(G, 166)),
    ("kswa_edge_b", lambda G: kswa_edge(167, True)),
    ("kswa_edge_w", lambda G: kswa_edge(168, False)),
    ("kswa_sat", lambda G: kswa_sat(G, 169, 2)),
    ("kswa_sat_a1", lambda G: kswa_sat(G, 170, 1)),
]


def make_kswa():
    if not oracle.ref_available():
        oracle.build(ref=True)
    tmp = tempfile.mkdtemp()
    try:
        with gzip.open(os.path.join(HERE, "g1.fa.gz"), "rb") as fh:
            from tests import golden_data
            g = golden_data.fasta_codes(fh.read())
        sets = [(name, lambda G, s=(seed, a, b, o, e): synth.make_kswa_tasks(G, 3000, seed=s[0], a=s[1], b=s[2], o=s[3],
                                                                             e=s[4]))
                for name, a, b, o, e, seed in KSWA_SETS] + KSWA_MORE
        for name, make in sets:
            kb = make(g)
            p = os.path.join(tmp, name + ".smat")
            synth.write_smat(p, kb)
            oracle.ref_kswa(p, os.path.join(tmp, name + ".smar"))
            for ext in (".smat", ".smar"):
                with open(os.path.join(tmp, name + ext), "rb") as fh:
                    gz_write(os.path.join(HERE, name + ext + ".gz"), fh.read())
    finally:
        shutil.rmtree(tmp)


# chains -> regions (mem_chain2aln_short / mem_chain2aln, software/bwamem.c:805-852,
# 1040-1188): the reference's own regions for every read of a seeding case,
# over the chains the matching filtered SMCH fixture holds
ALN_CASES = [("g1", "default", "std"), ("g1", "k14s20", "tight"), ("g2", "default", "std"), ("g2", "k14s20", "std")]


def make_aln():
    if not oracle.ref_available():
        oracle.build(ref=True)
    tmp = tempfile.mkdtemp()
    try:
        with open(os.path.join(HERE, "manifest.json")) as fh:
            manifest = json.load(fh)
        copts = {c["name"]: c for c in CHAIN_OPTS}
        for g in ("g1", "g2"):
            with gzip.open(os.path.join(HERE, g + ".fa.gz"), "rb") as fh, open(os.path.join(tmp, g + ".fa"), "wb") as o:
                o.write(fh.read())
            oracle.ref_index(os.path.join(tmp, g + ".fa"), os.path.join(tmp, g))
            with open(os.path.join(tmp, g + ".pac"), "rb") as fh:
                gz_write(os.path.join(HERE, g + ".pac.gz"), fh.read())
            rd = "r1.smrd" if g == "g1" else "r2.smrd"
            with gzip.open(os.path.join(HERE, rd + ".gz"), "rb") as fh, open(os.path.join(tmp, rd), "wb") as o:
                o.write(fh.read())
        out_cases = []
        for g, cname, oname in ALN_CASES:
            cases = manifest["cases"] if g == "g1" else manifest["g2"]["cases"]
            case = next(c for c in cases if c["name"] == cname)
            reads = synth.read_smrd(os.path.join(tmp, "r1.smrd" if g == "g1" else "r2.smrd"))
            sub = os.path.join(tmp, "sub.smrd")
            synth.write_smrd(sub, reads.subset(np.arange(case["n_reads"])))
            o, co = case["opt"], copts[oname]
            out = os.path.join(tmp, "a.smrg")
            subprocess.run([oracle.REF, "aln", os.path.join(tmp, g + ".bwt"), os.path.join(tmp, g + ".sa"),
                            os.path.join(tmp, g + ".pac"), sub, out, str(o["min_seed_len"]), str(o["split_factor"]),
                            str(o["split_width"]), str(o["start_width"]), str(MAX_OCC), str(co["w"]),
                            str(co["max_chain_gap"]), str(co["mask_level"]), str(co["drop_ratio"])], check=True)
            with open(out, "rb") as fh:
                data = fh.read()
            fn = f"{g}_{cname}_{oname}.smrg.gz"
            gz_write(os.path.join(HERE, fn), data)
            chain = next(c for c in case["chains"] if c["name"] == oname and c["filter"] == 1)
            out_cases.append(dict(genome=g, case=cname, chain_file=chain["file"], file=fn, w=co["w"],
                                  min_seed_len=o["min_seed_len"], sha256=hashlib.sha256(data).hexdigest()))
        manifest["aln"] = out_cases
        with open(os.path.join(HERE, "manifest.json"), "w") as fh:
            json.dump(manifest, fh, indent=1)
    finally:
        shutil.rmtree(tmp)
    make_aln_options()


# chains -> regions under non-default extension options (bwa mem -d / -L / -B /
# -O / -E / -A / -w / -k): read sets r3 (g1) and r4 (g2) of tests/aln_reads.py,
# their filtered chains, and the reference's regions under every option set of
# aln_reads.OPTION_SETS.  mem_chain reads opt->w and opt->min_seed_len too, so
# the w1 / w7 / k10 sets have chains of their own.
# genome, read set, seed, reads beside the 28 long ones
OPT_READS = [("g1", "r3", 301, 520), ("g2", "r4", 302, 255)]
# k10: the first 230 reads (seeds of 10 bp make several times the chains and regions)
OPT_CHAINS = [dict(name="std", min_seed_len=19, w=100), dict(name="k10", min_seed_len=10, w=100, n_reads=230),
              dict(name="w1", min_seed_len=19, w=1), dict(name="w7", min_seed_len=19, w=7)]
OPT_CHAIN_OF = {"k10": "k10", "w1": "w1", "w7": "w7"}   # option set -> chain set (the others: std)


def make_aln_options():
    from tests import aln_reads, golden_data
    if not oracle.ref_available():
        oracle.build(ref=True)
    tmp = tempfile.mkdtemp()
    try:
        with open(os.path.join(HERE, "manifest.json")) as fh:
            manifest = json.load(fh)
        std = next(c for c in CHAIN_OPTS if c["name"] == "std")
        sets, regs = {}, [f for f in manifest.get("aln", []) if "reads" not in f]
        for g, rname, seed, n in OPT_READS:
            with gzip.open(os.path.join(HERE, g + ".fa.gz"), "rb") as fh:
                fa_bytes = fh.read()
            with open(os.path.join(tmp, g + ".fa"), "wb") as o:
                o.write(fa_bytes)
            oracle.ref_index(os.path.join(tmp, g + ".fa"), os.path.join(tmp, g))
            reads = aln_reads.option_reads(golden_data.fasta_codes(fa_bytes), n, seed)
            smrd = os.path.join(tmp, rname + ".smrd")
            synth.write_smrd(smrd, reads)
            with open(smrd, "rb") as fh:
                data = fh.read()
            gz_write(os.path.join(HERE, rname + ".smrd.gz"), data)
            entry = dict(genome=g, file=rname + ".smrd.gz", n_reads=reads.n, seed=seed,
                         sha256=hashlib.sha256(data).hexdigest(), chains=[])
            subs = {}
            for co in OPT_CHAINS:
                nr = co.get("n_reads", reads.n)
                subs[co["name"]] = os.path.join(tmp, f"{rname}_{nr}.smrd")
                synth.write_smrd(subs[co["name"]], reads.subset(np.arange(nr)))
                case = dict(opt=dict(min_seed_len=co["min_seed_len"], split_factor=1.5, split_width=10, start_width=1))
                cd = ref_chain(tmp, subs[co["name"]], case, dict(std, w=co["w"]), 1, genome=g)
                fn = f"{g}_{rname}_{co['name']}_std_f1.smch.gz"
                gz_write(os.path.join(HERE, fn), cd)
                entry["chains"].append(dict(std, name=co["name"], w=co["w"], min_seed_len=co["min_seed_len"], file=fn,
                                            filter=1, n_reads=nr, sha256=hashlib.sha256(cd).hexdigest()))
            sets[rname] = entry
            for oname in aln_reads.OPTION_SETS:
                o = aln_reads.full_options(oname)
                chain = next(c for c in entry["chains"] if c["name"] == OPT_CHAIN_OF.get(oname, "std"))
                assert chain["w"] == o["w"] and chain["min_seed_len"] == o["min_seed_len"]
                out = os.path.join(tmp, "a.smrg")
                p = subprocess.run([oracle.REF, "aln", os.path.join(tmp, g + ".bwt"), os.path.join(tmp, g + ".sa"),
                                    os.path.join(tmp, g + ".pac"), subs[chain["name"]], out, str(o["min_seed_len"]), "1.5", "10", "1",
                                    str(MAX_OCC), str(o["w"]), str(std["max_chain_gap"]), str(std["mask_level"]),
                                    str(std["drop_ratio"])] +
                                   [str(o[k]) for k in ("a", "b", "o_del", "e_del", "o_ins", "e_ins", "zdrop",
                                                        "pen_clip5", "pen_clip3")])
                if p.returncode != 0:   # the reference itself faults on this set: left out, and said
                    print(f"ref_harness aln failed on {rname} {oname}: exit {p.returncode}", flush=True)
                    continue
                with open(out, "rb") as fh:
                    data = fh.read()
                fn = f"{g}_{rname}_{oname}.smrg.gz"
                gz_write(os.path.join(HERE, fn), data)
                regs.append(dict(genome=g, case=chain["name"], chain_file=chain["file"], file=fn, w=o["w"],
                                 min_seed_len=o["min_seed_len"], sha256=hashlib.sha256(data).hexdigest(),
                                 reads=rname, n_reads=chain["n_reads"], name=oname, opt=o,
                                 chain_sha256=chain["sha256"]))
        manifest["aln_reads"] = sets
        manifest["aln"] = regs
        with open(os.path.join(HERE, "manifest.json"), "w") as fh:
            json.dump(manifest, fh, indent=1)
    finally:
        shutil.rmtree(tmp)


# reads of 321 bp to 70 kbp (tests/long_reads.py class_reads): seeding, SA
# lookup and chains of the reference under the default options, in long/
LONG_SEED = 401
LONG_OPT = dict(min_seed_len=19, split_factor=1.5, split_width=10, start_width=1)


def make_long():
    from tests import golden_data, long_reads
    if not oracle.ref_available():
        oracle.build(ref=True)
    out_dir = os.path.join(HERE, "long")
    os.makedirs(out_dir, exist_ok=True)
    tmp = tempfile.mkdtemp()
    try:
        for name in ("g1.bwt", "g1.sa"):
            with gzip.open(os.path.join(HERE, name + ".gz"), "rb") as fh, open(os.path.join(tmp, name), "wb") as o:
                o.write(fh.read())
        with gzip.open(os.path.join(HERE, "g1.fa.gz"), "rb") as fh:
            G = golden_data.fasta_codes(fh.read())
        named = long_reads.class_reads(G, LONG_SEED)
        reads = long_reads.reads_of(named)
        smrd = os.path.join(tmp, "r5.smrd")
        synth.write_smrd(smrd, reads)
        with open(smrd, "rb") as fh:
            rd = fh.read()
        gz_write(os.path.join(out_dir, "r5.smrd.gz"), rd)
        out = os.path.join(tmp, "default.smgo")
        oracle.ref_smem(os.path.join(tmp, "g1.bwt"), smrd, out, **LONG_OPT)
        with open(out, "rb") as fh:
            data = fh.read()
        gz_write(os.path.join(out_dir, "g1_r5_default.smgo.gz"), data)
        parsed = synth.read_smgo(data)
        sa_out = os.path.join(tmp, "default.smsa")
        oracle.ref_sa(os.path.join(tmp, "g1.bwt"), os.path.join(tmp, "g1.sa"), out, sa_out,
                      min_seed_len=LONG_OPT["min_seed_len"], max_occ=MAX_OCC)
        with open(sa_out, "rb") as fh:
            sa_data = fh.read()
        gz_write(os.path.join(out_dir, "g1_r5_default.smsa.gz"), sa_data)
        case = dict(name="default", opt=LONG_OPT, n_reads=reads.n, sha256=hashlib.sha256(data).hexdigest(),
                    n_intv=int(sum(a.shape[0] for r in parsed for a in r)), n_calls=int(sum(len(r) for r in parsed)),
                    max_occ=MAX_OCC, sa_sha256=hashlib.sha256(sa_data).hexdigest(),
                    n_occ=int(sum(p.size for p in synth.read_smsa(sa_data))), chains=[])
        std = next(c for c in CHAIN_OPTS if c["name"] == "std")
        for filt in (0, 1):
            cd = ref_chain(tmp, smrd, case, std, filt)
            fn = f"g1_r5_default_std_f{filt}.smch.gz"
            gz_write(os.path.join(out_dir, fn), cd)
            case["chains"].append(dict(std, file=fn, filter=filt, sha256=hashlib.sha256(cd).hexdigest()))
        manifest = dict(genome="g1", seed=LONG_SEED,
                        reads=dict(file="r5.smrd.gz", n_reads=reads.n, n_bases=int(reads.codes.size),
                                   names=[n for n, _ in named], lens=[int(x) for x in reads.lens],
                                   sha256=hashlib.sha256(rd).hexdigest()),
                        cases=[case])
        with open(os.path.join(out_dir, "manifest.json"), "w") as fh:
            json.dump(manifest, fh, indent=1)
        print(json.dumps(manifest, indent=1))
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    if "--long-only" in sys.argv:
        make_long()
    elif "--aln-only" in sys.argv:
        make_aln()
    elif "--aln-options-only" in sys.argv:
        make_aln_options()
    elif "--ksw-only" in sys.argv:
        make_ksw()
        make_aln()
    elif "--ksw-gap0-only" in sys.argv:
        make_ksw_gap0()
    elif "--kswa-only" in sys.argv:
        make_kswa()
    elif "--chains-only" in sys.argv:
        chains_only()
    elif "--g2-only" in sys.argv:
        make_g2()
    else:
        main()
        make_g2()
        make_ksw()
        make_kswa()
