"""Golden data for the paired-end SAM text (the tail of mem_sam_pe, software/bwamem_pair.c:305-331,
through mem_aln2sam with a mate, software/bwamem.c:1219-1260).

    python tests/golden/make_golden_sampe.py

  sampe/sampe.fq.gz     interleaved pairs of 100 bp on the committed genome p1.fa.gz (two contigs
                        with repeats, tests/golden/make_golden_pair.py: make_p1); names of 2 to 21
                        bytes, one per pair, and qualities that vary along and between the reads
  sampe/sampe.smrg.gz   the reference's regions of every read before mem_sort_and_dedup
                        (ref_harness aln)
  sampe/sampe.sam.gz    the reference's SAM (ref_harness mem)
  sampe/sampe.json      the kinds of pairs, the counts of the line classes below, and the pairs the
                        restated chain leaves to the host

Kinds (KINDS below): ordinary FR pairs of insert 350 +- 30; either end or both replaced by random
bases; the mate taken from the other contig; FF pairs; pairs with their ends swapped; a first read
that is part one contig, part the other (a supplementary line), its mate beside either part;
inserts of 100 and 101.  Every fragment lies inside its contig.

The set is written only if the reference's SAM holds at least MIN_CLASS lines in every class of
tests/sampe_chain.CLASSES, the restated chain with tests/samtext_pe_ref.py gives every line of every
pair it keeps, byte for byte, and it leaves at most pair_chain.MAX_HOST_FRACTION of the pairs to
the host.
"""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem-harp2_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # shared helpers between test modules, as tests/conftest.py adds it
sys.path.insert(0, HERE)

import make_golden_pair as MP  # noqa: E402
from oracle import oracle  # noqa: E402
from smemgpu import synth  # noqa: E402

OUT = os.path.join(HERE, "sampe")
L = 100
KINDS = (("fr", 160), ("end1_random", 14), ("end2_random", 14), ("both_random", 12), ("other_contig", 15), ("ff", 15),
         ("swapped", 15), ("chimeric", 40), ("insert_100", 10), ("insert_101", 10))


def name_of(p):
    """pair p's name: 2 to 21 bytes, the index first"""
    return f"q{p}" + (":" + "abcdefghijklmnopq"[:p % 17] if p % 3 else "")


def qual_of(r, n):
    """read r's qualities: neither constant nor palindromic"""
    return (33 + (7 * r + 3 * np.arange(n)) % 41).astype(np.uint8)


def make_reads(G):
    rng = np.random.default_rng(7401)
    C = MP.CONTIG
    ins = lambda: int(np.clip(np.rint(rng.normal(350, 30)), 250, 450))   # noqa: E731
    place = lambda c, n: c * C + int(rng.integers(100, C - n - 100))     # noqa: E731  (the fragment inside contig c)
    plain = lambda c, k: c * C + 38_050 + 37 * k                         # noqa: E731  (no feature past 38 000)
    rand = lambda: rng.integers(0, 4, size=L).astype(np.uint8)           # noqa: E731
    reads, kinds = [], []
    for kind, count in KINDS:
        for k in range(count):
            c, n = int(rng.integers(0, 2)), ins()
            a, b = MP.pair_reads(G, place(c, n), n, 1, L)
            if kind == "end1_random":
                a = rand()
            elif kind == "end2_random":
                b = rand()
            elif kind == "both_random":
                a, b = rand(), rand()
            elif kind == "other_contig":
                b = MP.rc(G[place(1 - c, L):][:L])
            elif kind == "ff":
                a, b = MP.pair_reads(G, place(c, n), n, 0, L)
            elif kind == "swapped":
                a, b = b, a
            elif kind == "chimeric":     # the first read: `cut` bases beside the mate's fragment, the rest from the other contig
                cut = (45, 50, 55, 60, 40)[k % 5]
                far = G[plain(1 - c, k):][:L]
                a = np.concatenate([a[:cut], far[cut:]]) if k % 2 == 0 else np.concatenate([far[:L - cut], a[L - cut:]])
            elif kind.startswith("insert_"):
                n = int(kind[7:])
                a, b = MP.pair_reads(G, place(c, n), n, 1, L)
            assert a.size == L and b.size == L
            reads += [a, b]
            kinds.append(kind)
    return reads, kinds


def run_reference(fa_bytes, reads):
    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "p1.fa")
        with open(fa, "wb") as fh:
            fh.write(fa_bytes)
        subprocess.run([MP.REF, "index", fa, fa], check=True, capture_output=True)
        fq = os.path.join(d, "pe.fq")
        acgt = np.frombuffer(b"ACGTN", dtype=np.uint8)
        with open(fq, "wb") as fh:
            for r, x in enumerate(reads):
                fh.write(b"@" + name_of(r // 2).encode() + b"\n" + acgt[x].tobytes() + b"\n+\n" + qual_of(r, x.size).tobytes() + b"\n")
        p = subprocess.run([MP.REF, "mem", fa, fq, "1", "1", "1"], check=True, capture_output=True)
        lens = np.array([x.size for x in reads], dtype=np.int32)
        R = synth.Reads(lens, np.concatenate(reads).astype(np.uint8), np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]))
        smrd, smrg = os.path.join(d, "pe.smrd"), os.path.join(d, "pe.smrg")
        synth.write_smrd(smrd, R)
        subprocess.run([MP.REF, "aln", fa + ".bwt", fa + ".sa", fa + ".pac", smrd, smrg, "19", "1.5", "10", "1", "10000",
                        "100", "10000", "0.5", "0.5"], check=True, capture_output=True)
        with open(smrg, "rb") as fh:
            smrg_bytes = fh.read()
        with open(fq, "rb") as fh:
            fq_bytes = fh.read()
    return fq_bytes, smrg_bytes, p.stdout


def main():
    if not oracle.ref_available():
        oracle.build(ref=True)
    from tests import pair_chain as PC, sampe_chain as SC
    with gzip.open(os.path.join(HERE, "p1.fa.gz"), "rb") as fh:
        fa = fh.read()
    G = PC.genome("p1")[0]
    reads, kinds = make_reads(G)
    fq, smrg, sam = run_reference(fa, reads)
    man = dict(genome="p1", options="default", pairs=len(kinds), read_len=L, kinds={k: n for k, n in KINDS})
    cls = SC.classes(sam)
    short = {k: v for k, v in cls.items() if v < SC.MIN_CLASS}
    if short:
        raise SystemExit(f"sampe: fewer than {SC.MIN_CLASS} lines in {short} (all: {cls})")
    F = SC.make(man, fq, smrg, sam)
    got = SC.texts(F, SC.restated(F))
    host = [p for p in range(len(kinds)) if got[2 * p] is None]
    bad = [(r, kinds[r // 2]) for r in range(len(got)) if got[r] is not None and got[r] != F["want"][r]]
    if bad:
        r = bad[0][0]
        raise SystemExit(f"sampe: the restatement differs from the reference's SAM in {len(bad)} reads: {bad[:8]}\n{got[r]}\n{F['want'][r]}")
    if len(host) > PC.MAX_HOST_FRACTION * len(kinds):
        raise SystemExit(f"sampe: {len(host)} of {len(kinds)} pairs are left to the host: {host[:10]}")
    man.update(classes=cls, left_to_host=host, sam_lines=sum(1 for x in sam.split(b"\n") if x and not x.startswith(b"@")))
    os.makedirs(OUT, exist_ok=True)
    for ext, data in ((".fq.gz", fq), (".smrg.gz", smrg), (".sam.gz", sam)):
        with open(os.path.join(OUT, "sampe" + ext), "wb") as fh:
            fh.write(gzip.compress(data, 9, mtime=0))
    with open(os.path.join(OUT, "sampe.json"), "w") as fh:
        json.dump(man, fh, indent=1)
    print("sampe", cls, "host", host)


if __name__ == "__main__":
    main()
