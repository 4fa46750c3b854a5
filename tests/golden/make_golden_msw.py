"""Golden data for mate rescue (mem_matesw, software/bwamem_pair.c:109-175):
the long-target ksw_align2 problems and one paired-end set.

    python tests/golden/make_golden_msw.py              # all three
    python tests/golden/make_golden_msw.py --kswa-only
    python tests/golden/make_golden_msw.py --pairs-only
    python tests/golden/make_golden_msw.py --hand-only

  kswa_msw_a<1|2>.smat.gz / .smar.gz
        ksw_align2 problems with targets of 257..MAX_TLEN bases under
        mem_opt_init's scoring (a = 1) and -A 2 scaling (a = 2), and the
        compiled reference's own ksw_align2 on each (ref_harness kswa,
        software/ksw.c:342); at most 600 in all.
  kswa_msw.json
        where each group of problems sits in its set, and for the groups
        built around the suboptimal list what they were built to show
  msw/g1_pe.fq.gz, msw/g1_pe.sam.gz, msw/g1_pe.smrg.gz, msw/g1_pe.json
        the paired-end set on g1 (make_pairs below), the reference's SAM
        (ref_harness mem ... 1), its regions of every read before
        mem_sort_and_dedup (ref_harness aln) and what it printed about insert
        sizes: the proper-pair bounds of FR and the orientations it skipped
  msw/hand/<batch>.smmo.gz, msw/hand/manifest.json
        the reference's own mem_matesw (ref_harness msw: the loop of
        software/bwamem_pair.c:252-263 around it) on every hand-built batch of
        tests/matesw_data.fixtures(): each read's list afterwards and the summed
        returns per pair (SMMO, oracle/ref_harness.c).  The inputs are not stored:
        the manifest names the builder, the bounds, the options, the pair count and
        the sha256 of the harness's input, which tests/test_matesw.py recomputes
        from the builders.  Batches:
          all_<o>, fr_<o>      build (PES_ALL) and build_fr (PES_FR) under
                               o = base, a2, one_anchor, no_margin, no_anchor
          <case>_<o>           each case of build_edges -- long, roll, both, n, lpac,
                               window, equal, short -- under o = base, a2, one_anchor
          lpac<l>_base         the lpac case on genomes of l = 200001, 200002, 200003
"""
import gzip
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem-harp2_amd"))
sys.path.insert(0, ROOT)

from oracle import oracle  # noqa: E402
from smemgpu import synth  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
MAX_TLEN = 2048   # SMEM_KSWA_MAX_TLEN
X_BYTE, X_STOP, X_SUBO, X_START = synth.KSW_XBYTE, synth.KSW_XSTOP, synth.KSW_XSUBO, synth.KSW_XSTART
GRID_TLEN = [257, 319, 320, 321, 511, 512, 513, 1000, MAX_TLEN - 1, MAX_TLEN]
GRID_QLEN = [1, 16, 17, 64, 65, 150, 250, 256]
PART = 40         # bases of the query the `tie` blocks repeat


def gz_write(path, data: bytes):
    with gzip.GzipFile(path, "wb", mtime=0) as fh:
        fh.write(data)


def _batch(items, a):
    tasks = np.zeros(len(items), dtype=synth.KSWA_TASK)
    qo = to = 0
    for k, (q, t, xtra) in enumerate(items):
        assert 1 <= q.size <= 256 and t.size <= MAX_TLEN
        tasks[k] = (qo, to, q.size, t.size, xtra, 0)
        qo += q.size
        to += t.size
    cat = lambda xs: np.concatenate([np.asarray(x, dtype=np.uint8) for x in xs])
    return synth.KswBatch(tasks, cat([i[0] for i in items]), cat([i[1] for i in items]), synth.bwa_scmat(a, 4 * a),
                          6 * a, a, 6 * a, a)


def _rc(x):
    return np.where(x < 4, 3 - x, 4)[::-1].astype(np.uint8)


def _rnd(rng, n):
    return rng.integers(0, 4, size=n).astype(np.uint8)


def _msw_xtra(l_ms, a, min_seed_len=19):
    """mem_matesw's flags (software/bwamem_pair.c:143)"""
    return X_SUBO | X_START | (X_BYTE if l_ms * a < 250 else 0) | (min_seed_len * a)


def kswa_msw(G, seed, a):
    """(KswBatch, groups, facts) of one scoring.  Groups, in order:
    grid    every target length around a multiple of the 64-row fetch and at the
            limit against every query length around the vector widths and the
            wave's chunk; at a = 1 each both byte-scored and 16-bit, at a = 2 by
            mem_matesw's rule (queries from 125 bp on are 16-bit)
    rescue  mem_matesw's shape: a read of 100..250 bp with substitutions and
            indels against a window of 400..1500 bp that holds it, every second
            one reverse-complemented (both, as the rescue of a reverse mate is)
    tandem  `A` and `AC` against (AC)^k with a threshold of 1: the list b gets an
            entry every second row -- 150, 300 and tlen / 2 = 1024 entries
    late    the query's best copy early in the target, a weaker copy in its last
            part, far outside the best hit's window, and a threshold of 4 so that
            chance rows fill the list in between: score2 / te2 are a late entry
    tie     two identical blocks (N, the query's first 40 bases, N) on either
            side of the full copy, or both behind it: two list entries of the
            same score, of which the strict > scan keeps the first"""
    rng = np.random.default_rng(seed)
    items, groups, facts = [], {}, {}

    def group(name, new):
        groups[name] = [len(items), len(items) + len(new)]
        items.extend(new)

    new = []
    for tlen in GRID_TLEN:
        for qlen in GRID_QLEN:
            for byte in ((True, False) if a == 1 else (qlen * a < 250,)):
                q = _rnd(rng, qlen)
                off = int(rng.integers(0, tlen - qlen + 1))
                if off + qlen > tlen - 2 and rng.random() < 0.5:
                    off = tlen - qlen      # the hit ends in the last row
                t = np.concatenate([_rnd(rng, off), q, _rnd(rng, tlen - qlen - off)])
                if qlen >= 16:
                    m = synth._mutated_copy(q, rng, 0.06, 0.02)
                    q = np.concatenate([m, _rnd(rng, qlen)])[:qlen]
                new.append((q, t, X_SUBO | X_START | (X_BYTE if byte else 0) | 19 * a))
    group("grid", new)

    new = []
    for k in range(110):
        ql = int(rng.integers(100, 251))
        wl = int(rng.integers(400, 1501))
        pos = int(rng.integers(2000, G.size - 4000))
        t = G[pos:pos + wl].copy()
        at = int(rng.integers(0, wl - ql - 20))
        q = synth._mutated_copy(t[at:at + ql + 20], rng, float(rng.choice([0.0, 0.02, 0.05, 0.1])),
                                float(rng.choice([0.0, 0.01, 0.03])))[:ql]
        if k % 2:
            q, t = _rc(q), _rc(t)
        new.append((q, t, _msw_xtra(q.size, a)))
    group("rescue", new)

    new = []
    for k in (150, 300, MAX_TLEN // 2):
        ac = np.tile(np.array([0, 1], np.uint8), k)
        new.append((ac[:1].copy(), ac, X_SUBO | X_START | X_BYTE | 1))
        new.append((ac[:2].copy(), ac, X_SUBO | X_START | X_BYTE | 1))
    group("tandem", new)
    facts["tandem_entries"] = [150, 150, 300, 300, MAX_TLEN // 2, MAX_TLEN // 2]

    new, late_from = [], []
    for k in range(20):
        ql = int(rng.integers(60, 121))
        tlen = int(rng.integers(900, MAX_TLEN + 1))
        q = _rnd(rng, ql)
        weak = synth._mutated_copy(q, rng, 0.08, 0.0)
        head = int(rng.integers(0, 100))
        tail = int(rng.integers(0, 30))
        mid = tlen - head - ql - weak.size - tail
        t = np.concatenate([_rnd(rng, head), q, _rnd(rng, mid), weak, _rnd(rng, tail)])
        late_from.append(int(head + ql + mid))
        byte = ql * a < 250 and k % 2 == 0
        new.append((q, t, X_SUBO | X_START | (X_BYTE if byte else 0) | 4))
    group("late", new)
    facts["late_from"] = late_from

    new, tie_first, tie_second = [], [], []
    for k in range(20):
        ql = int(rng.integers(80, 151))
        q = _rnd(rng, ql)
        n5 = np.full(5, 4, np.uint8)
        blk = np.concatenate([n5, q[:PART], n5])
        g = [int(x) for x in rng.integers(30, 400, size=4)]
        if k % 2 == 0:
            parts = [_rnd(rng, g[0]), blk, _rnd(rng, g[1]), q, _rnd(rng, g[2]), blk, _rnd(rng, g[3])]
            b1, b2 = g[0], g[0] + blk.size + g[1] + ql + g[2]
        else:
            parts = [_rnd(rng, g[0]), q, _rnd(rng, g[1]), blk, _rnd(rng, g[2]), blk, _rnd(rng, g[3])]
            b1 = g[0] + ql + g[1]
            b2 = b1 + blk.size + g[2]
        t = np.concatenate(parts)
        tie_first.append(b1 + 5 + PART - 1)    # the row of the first block's last query base
        tie_second.append(b2 + 5 + PART - 1)
        new.append((q, t, _msw_xtra(ql, a)))
    group("tie", new)
    facts["tie_first"], facts["tie_second"] = tie_first, tie_second
    return _batch(items, a), groups, facts


def make_kswa():
    if not oracle.ref_available():
        oracle.build(ref=True)
    from tests import golden_data
    with gzip.open(os.path.join(HERE, "g1.fa.gz"), "rb") as fh:
        G = golden_data.fasta_codes(fh.read())
    meta = {"max_tlen": MAX_TLEN}
    tmp = tempfile.mkdtemp()
    try:
        for a, seed in ((1, 181), (2, 182)):
            name = f"kswa_msw_a{a}"
            kb, groups, facts = kswa_msw(G, seed, a)
            p = os.path.join(tmp, name + ".smat")
            synth.write_smat(p, kb)
            oracle.ref_kswa(p, os.path.join(tmp, name + ".smar"))
            for ext in (".smat", ".smar"):
                with open(os.path.join(tmp, name + ext), "rb") as fh:
                    gz_write(os.path.join(HERE, name + ext + ".gz"), fh.read())
            meta[name] = {"n": int(kb.tasks.size), "groups": groups, **facts}
            print(name, kb.tasks.size, groups, flush=True)
    finally:
        shutil.rmtree(tmp)
    with open(os.path.join(HERE, "kswa_msw.json"), "w") as fh:
        json.dump(meta, fh, indent=1)


# ---- the paired-end set ------------------------------------------------------
N_PLAIN, N_UNSEEDED, READ_LEN = 250, 60, 150
MIN_RESCUED = 40


def make_pairs_reads(G):
    """N_PLAIN ordinary pairs (150 bp, insert N(500, 50), 2 % substitutions): enough for the
    reference to infer FR; then N_UNSEEDED error-free pairs whose second mate gets a
    substitution at every tenth base (5, 15, ...): no exact match of 19 bp is left, so the mate
    gets no seed and no region of its own, while its local score, about 135 - 60 = 75, is well
    above the output threshold of 30 -- only mate rescue can place it"""
    plain = synth.make_pairs(G, N_PLAIN, READ_LEN, seed=211, sub_rate=0.02, n_rate=0.0)
    hard = synth.make_pairs(G, N_UNSEEDED, READ_LEN, seed=212, sub_rate=0.0, n_rate=0.0)
    codes = hard.codes.copy().reshape(-1, READ_LEN)
    rng = np.random.default_rng(213)
    for k in range(1, codes.shape[0], 2):
        at = np.arange(5, READ_LEN, 10)
        codes[k, at] = (codes[k, at] + rng.integers(1, 4, size=at.size)) & 3
    hard = synth.Reads(hard.lens, codes.reshape(-1).astype(np.uint8), hard.offs)
    return synth.concat_reads([plain, hard])


def parse_pestat(stderr: str):
    """mem_pestat's messages (software/bwamem_pair.c:55-106) -> per orientation low, high, failed"""
    pes = [dict(low=0, high=0, failed=1) for _ in range(4)]
    cur = None
    for line in stderr.split("\n"):
        m = re.search(r"analyzing insert size distribution for orientation ([FR])([FR])", line)
        if m:
            cur = "FR".index(m.group(1)) << 1 | "FR".index(m.group(2))
        m = re.search(r"low and high boundaries for proper pairs: \((-?\d+), (-?\d+)\)", line)
        if m and cur is not None:
            pes[cur] = dict(low=int(m.group(1)), high=int(m.group(2)), failed=0)
        m = re.search(r"skip orientation ([FR])([FR])", line)
        if m:
            pes["FR".index(m.group(1)) << 1 | "FR".index(m.group(2))]["failed"] = 1
    return pes


def make_pairs():
    if not oracle.ref_available():
        oracle.build(ref=True)
    from tests import golden_data
    out = os.path.join(HERE, "msw")
    os.makedirs(out, exist_ok=True)
    with gzip.open(os.path.join(HERE, "g1.fa.gz"), "rb") as fh:
        fa_bytes = fh.read()
    G = golden_data.fasta_codes(fa_bytes)
    reads = make_pairs_reads(G)
    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "g1.fa")
        with open(fa, "wb") as fh:
            fh.write(fa_bytes)
        subprocess.run([REF, "index", fa, fa], check=True, capture_output=True)
        fq = os.path.join(d, "pe.fq")
        acgtn = np.frombuffer(b"ACGTN", dtype=np.uint8)
        with open(fq, "wb") as fh:
            for i in range(reads.n):
                seq = acgtn[np.minimum(reads.read(i), 4)].tobytes()
                fh.write(b"@p%d\n" % (i // 2) + seq + b"\n+\n" + b"I" * len(seq) + b"\n")
        p = subprocess.run([REF, "mem", fa, fq, "1", "1", "1"], check=True, capture_output=True)
        pes = parse_pestat(p.stderr.decode(errors="replace"))
        # the reference's regions of every read before mem_sort_and_dedup (its mem_chain2aln loop)
        smrd = os.path.join(d, "pe.smrd")
        synth.write_smrd(smrd, reads)
        smrg = os.path.join(d, "pe.smrg")
        subprocess.run([REF, "aln", fa + ".bwt", fa + ".sa", fa + ".pac", smrd, smrg, "19", "1.5", "10", "1", "10000",
                        "100", "10000", "0.5", "0.5"], check=True, capture_output=True)
        with open(smrg, "rb") as fh:
            smrg_bytes = fh.read()
        with open(fq, "rb") as fh:
            fq_bytes = fh.read()
    regs, reg_off = golden_data.smrg_parse(smrg_bytes)
    none = np.diff(reg_off.astype(np.int64)) == 0
    mapped = {}
    for line in p.stdout.decode().split("\n"):
        if line and not line.startswith("@"):
            f = line.split("\t")
            flag = int(f[1])
            if not flag & 0x900:
                mapped[2 * int(f[0][1:]) + (1 if flag & 0x80 else 0)] = not flag & 4
    rescued = [r for r in range(reads.n) if none[r] and mapped.get(r)]
    print("pes", pes, "reads without a region", int(none.sum()), "of them mapped", len(rescued), flush=True)
    if pes[1]["failed"] or any(not pes[r]["failed"] for r in (0, 2, 3)):
        raise SystemExit("the reference did not infer FR alone")
    if len(rescued) < MIN_RESCUED:
        raise SystemExit(f"only {len(rescued)} reads without a region are mapped: the set would pin nothing")
    gz_write(os.path.join(out, "g1_pe.fq.gz"), fq_bytes)
    gz_write(os.path.join(out, "g1_pe.sam.gz"), p.stdout)
    gz_write(os.path.join(out, "g1_pe.smrg.gz"), smrg_bytes)
    with open(os.path.join(out, "g1_pe.json"), "w") as fh:
        json.dump({"genome": "g1", "pairs": reads.n // 2, "read_len": READ_LEN, "pes": pes,
                   "reads_without_region": int(none.sum()), "of_them_mapped": len(rescued)}, fh, indent=1)


# ---- the reference's mem_matesw on the hand-built pairs ---------------------------------------
def make_hand():
    """every batch of tests/matesw_data.fixtures() through `ref_harness msw`: the lists afterwards and
    the summed returns (SMMO), and in manifest.json what each batch was and a digest of what went in"""
    import dataclasses
    import hashlib
    from tests import matesw_data as D
    if not oracle.ref_available():
        oracle.build(ref=True)
    out = os.path.join(HERE, "msw", "hand")
    os.makedirs(out, exist_ok=True)
    man = {}
    with tempfile.TemporaryDirectory() as d:
        for name, (G, l_pac, case) in D.fixtures().items():
            data = D.smmi_bytes(G, l_pac, case)
            with open(os.path.join(d, "in.smmi"), "wb") as fh:
                fh.write(data)
            subprocess.run([REF, "msw", os.path.join(d, "in.smmi"), os.path.join(d, "out.smmo")], check=True)
            with open(os.path.join(d, "out.smmo"), "rb") as fh:
                res = fh.read()
            regs, reg_off, n = D.smmo_parse(res)
            gz_write(os.path.join(out, name + ".smmo.gz"), res)
            builder = "build" if name.startswith("all_") else "build_fr" if name.startswith("fr_") else \
                "build_edges:" + name.split("_")[0].rstrip("0123456789")
            man[name] = {"builder": builder, "l_pac": int(l_pac), "pes": [[p.low, p.high, p.failed] for p in case.pes],
                         "opt": dataclasses.asdict(case.opt), "pairs": len(case.pairs.group),
                         "regions_in": int(sum(len(x) for x in case.pairs.lists)), "regions_out": int(regs.size),
                         "n_sw": int(n.sum()), "input_sha256": hashlib.sha256(data).hexdigest()}
            print(name, man[name]["pairs"], "pairs", regs.size, "regions", int(n.sum()), "SWs", flush=True)
    with open(os.path.join(out, "manifest.json"), "w") as fh:
        json.dump(man, fh, indent=1)


if __name__ == "__main__":
    if "--hand-only" in sys.argv:
        make_hand()
        sys.exit(0)
    if "--pairs-only" not in sys.argv:
        make_kswa()
    if "--kswa-only" not in sys.argv:
        make_pairs()
    if "--kswa-only" not in sys.argv and "--pairs-only" not in sys.argv:
        make_hand()
