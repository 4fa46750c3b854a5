"""Golden data for insert-size statistics and pairing (mem_pestat, mem_pair and the decision
block of mem_sam_pe, software/bwamem_pair.c:46-107, 177-236, 264-304, 321-326).

    python tests/golden/make_golden_pair.py

  pair/<set>.fq.gz     interleaved pairs
  pair/<set>.smrg.gz   the reference's regions of every read before mem_sort_and_dedup
                       (ref_harness aln)
  pair/<set>.json      what mem_pestat printed while ref_harness mem ran the set (candidate
                       counts, percentiles, both pairs of bounds, mean and std.dev as printed,
                       the "skip orientation" lines of either kind), and what the restatement's
                       Trace reached
  pair/<set>.sam.gz    the reference's SAM (pairing sets only)
  p1.fa.gz             the pairing sets' genome (make_p1 below): two contigs of 40 kbp with exact
                       duplicates, copies with 3 and with 4 substitutions per 100 bases, and
                       tandem arrays

pestat sets, on g1 (each refused unless the reference's messages show what it was built for):
  fr_only, fr_rf (both survive), ratio (RF has at least 10 candidates and the 5 % rule removes
  it), nine_ten (FF with 9 candidates beside RF with 10), heavy (a wide spread inside the outlier
  bounds: line 94 replaces low by avg - 4 std), short (50 bp reads, inserts from the read length
  up: low clamps to 1), repeats (reads from g1's repeated segments: second regions that overlap
  the first, on both sides of cal_sub's tests).
pairing sets, on p1: rep under the default options and rep_a2 under `-A 2`, the same reads.  Beside
200 ordinary pairs they hold pairs with an end in an exact duplicate (the pair chooses between two
equal hits), in a copy with 3 substitutions (the pair prefers a region that is not the end's
best) or with 4 (the unpaired alignment is preferred), in a tandem array (several candidate
pairs), with a chimeric end (two primary regions: is_multi) and with ends from unrelated places
(no candidate).  tests/pair_chain.py runs regions -> sort_and_dedup -> pestat -> matesw_ref ->
mark_primary_se -> pair -> reg2aln_ref; a set is written only if every pair the chain keeps gives
both primary lines' FLAG & 2, strand, RNAME / POS, MAPQ and XS, at most 2 % of the pairs are left
to the host, and the Trace shows at least ten pairs in each group of pair_chain.GROUPS.  Ties
decided by the hash are counted in the .json.
"""
import gzip
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem-harp2_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # shared helpers between test modules, as tests/conftest.py adds it

from oracle import oracle  # noqa: E402
from smemgpu import synth  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
OUT = os.path.join(HERE, "pair")
DIRS = ("FF", "FR", "RF", "RR")


def rc(x):
    return np.where(x < 4, 3 - x, 4)[::-1].astype(np.uint8)


def pair_reads(G, pos, ins, d, L):
    """the two mates of a fragment G[pos:pos + ins] in orientation d (mem_infer_dir's numbering)"""
    a, b = G[pos:pos + L], G[pos + ins - L:pos + ins]
    return {0: (a, b), 1: (a, rc(b)), 2: (rc(a), b), 3: (b, a)}[d]


def build(G, spec, L, seed):
    """spec: [(orientation, [insert sizes])] -> list of reads, two per pair; fragments from unique
    places of the first contig"""
    rng = np.random.default_rng(seed)
    reads = []
    for d, sizes in spec:
        for ins in sizes:
            pos = int(rng.integers(1000, 80_000))
            reads += list(pair_reads(G, pos, int(ins), d, L))
    return reads


def parse_pestat(stderr):
    out = dict(n_cand=None, dirs={}, few=[], ratio=[])
    cur = None
    for line in stderr.split("\n"):
        m = re.search(r"candidate unique pairs for \(FF, FR, RF, RR\): \((\d+), (\d+), (\d+), (\d+)\)", line)
        if m:
            out["n_cand"] = [int(x) for x in m.groups()]
        m = re.search(r"skip orientation ([FR][FR]) as there are not enough pairs", line)
        if m:
            out["few"].append(DIRS.index(m.group(1)))
            continue
        m = re.search(r"skip orientation ([FR][FR])\s*$", line)
        if m:
            out["ratio"].append(DIRS.index(m.group(1)))
        m = re.search(r"analyzing insert size distribution for orientation ([FR][FR])", line)
        if m:
            cur = str(DIRS.index(m.group(1)))
            out["dirs"][cur] = {}
        for key, pat in (("pct", r"\(25, 50, 75\) percentile: \((-?\d+), (-?\d+), (-?\d+)\)"),
                         ("bounds1", r"boundaries for computing mean and std.dev: \((-?\d+), (-?\d+)\)"),
                         ("bounds", r"boundaries for proper pairs: \((-?\d+), (-?\d+)\)")):
            m = re.search(pat, line)
            if m:
                out["dirs"][cur][key] = [int(x) for x in m.groups()]
        m = re.search(r"mean and std.dev: \(([-0-9.a-z]+), ([-0-9.a-z]+)\)", line)
        if m:
            out["dirs"][cur]["mean_std"] = [m.group(1), m.group(2)]
    return out


A2_MEM = ["@PG\tID:bwa\tPN:bwa\tVN:0.7.8-r455", "-A", "2"]
A2_ALN = ["2", "8", "12", "2", "12", "2", "200", "10", "10"]   # a b o_del e_del o_ins e_ins zdrop pen_clip5 pen_clip3


def run_reference(fa_bytes, reads, want_sam, a2=False):
    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "g1.fa")
        with open(fa, "wb") as fh:
            fh.write(fa_bytes)
        subprocess.run([REF, "index", fa, fa], check=True, capture_output=True)
        fq = os.path.join(d, "pe.fq")
        acgtn = np.frombuffer(b"ACGTN", dtype=np.uint8)
        with open(fq, "wb") as fh:
            for i, r in enumerate(reads):
                seq = acgtn[np.minimum(r, 4)].tobytes()
                fh.write(b"@p%d\n" % (i // 2) + seq + b"\n+\n" + b"I" * len(seq) + b"\n")
        p = subprocess.run([REF, "mem", fa, fq, "1", "1", "1"] + (A2_MEM if a2 else []), check=True, capture_output=True)
        lens = np.array([r.size for r in reads], dtype=np.int32)
        R = synth.Reads(lens, np.concatenate(reads).astype(np.uint8), np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]))
        smrd, smrg = os.path.join(d, "pe.smrd"), os.path.join(d, "pe.smrg")
        synth.write_smrd(smrd, R)
        subprocess.run([REF, "aln", fa + ".bwt", fa + ".sa", fa + ".pac", smrd, smrg, "19", "1.5", "10", "1", "10000",
                        "100", "10000", "0.5", "0.5"] + (A2_ALN if a2 else []), check=True, capture_output=True)
        with open(smrg, "rb") as fh:
            smrg_bytes = fh.read()
        with open(fq, "rb") as fh:
            fq_bytes = fh.read()
    return fq_bytes, smrg_bytes, parse_pestat(p.stderr.decode(errors="replace")), p.stdout if want_sam else None


def repeated_places(G, k=60, limit=400):
    """starts of k-mers of g1 that occur more than once (either strand not considered)"""
    seen, out = {}, []
    for i in range(0, G.size - k, 7):
        key = G[i:i + k].tobytes()
        if key in seen:
            out.append((seen[key], i))
        else:
            seen[key] = i
    return out[:limit]


def placed_unique(G, reads, L):
    """no 30-mer of any read occurs twice in g1: every pair will be a candidate"""
    seen = {}
    for i in range(G.size - 30):
        k = G[i:i + 30].tobytes()
        seen[k] = seen.get(k, 0) + 1
    for r in reads:
        for x in (r, rc(r)):
            for j in range(0, L - 30, 10):
                if seen.get(x[j:j + 30].tobytes(), 0) > 1:
                    return False
    return True


def sets(G):
    rng = np.random.default_rng(4401)
    norm = lambda n, m=400, s=40: np.clip(np.rint(rng.normal(m, s, size=n)), 150, 2000).astype(int)   # noqa: E731
    S = {}
    S["fr_only"] = (build(G, [(1, norm(300))], 100, 1), 100)
    S["fr_rf"] = (build(G, [(1, norm(200)), (2, norm(100, 700, 60))], 100, 2), 100)
    S["ratio"] = (build(G, [(1, norm(300)), (2, norm(12, 700, 60))], 100, 3), 100)
    for seed in range(4, 400, 50):   # the counts are the reference's: take the first placement that gives 9 and 10
        S["nine_ten"] = (build(G, [(1, norm(100)), (2, norm(10, 700, 60)), (0, norm(9, 600, 30))], 100, seed), 100)
        if placed_unique(G, S["nine_ten"][0], 100):
            break
    S["heavy"] = (build(G, [(1, [830] * 58 + [1300 + 2 * k for k in range(125)] + [2020] * 58)], 100, 5), 100)
    S["short"] = (build(G, [(1, rng.integers(50, 121, size=200))], 50, 6), 50)
    reads = build(G, [(1, norm(150))], 100, 7)
    for a, b in repeated_places(G):
        for p in (a, b):
            if 600 < p < G.size - 600:
                reads += list(pair_reads(G, p - 20, int(norm(1)[0]), 1, 100))
    S["repeats"] = (reads[:1200], 100)
    return S


def shows(name, msg, tr):
    """the case a set was built for, in the reference's own messages"""
    alive = [int(d) for d in msg["dirs"] if int(d) not in msg["ratio"]]
    if name == "fr_only":
        return alive == [1]
    if name == "fr_rf":
        return sorted(alive) == [1, 2]
    if name == "ratio":
        return msg["ratio"] == [2] and msg["n_cand"][2] >= 10
    if name == "nine_ten":
        return msg["n_cand"][0] == 9 and msg["n_cand"][2] == 10 and 0 in msg["few"] and 2 in alive
    if name == "heavy":
        p25, _, p75 = msg["dirs"]["1"]["pct"]
        return msg["dirs"]["1"]["bounds"][0] != max(1, int(p25 - 3.0 * (p75 - p25) + .499)) and tr.low_cap == [1]
    if name == "short":
        return msg["dirs"]["1"]["bounds"][0] == 1 and msg["dirs"]["1"]["bounds1"][0] == 1
    if name == "repeats":
        return tr.not_unique >= 5 and tr.sub_kept >= 3
    return False


# ---- the pairing sets' genome and reads --------------------------------------
N_FEAT, SLOT, CONTIG = 24, 1500, 40_000


def make_p1():
    """(codes, FASTA bytes, features): contig c0 holds the sources at 2000 + 1500 i, contig c1 the
    copies at the same offsets; feature i is, by i % 4: an exact duplicate of 300 bases, a copy with a
    substitution every 34 bases (3 per 100), one with a substitution every 25 bases (4 per 100), or --
    on c0 only -- a tandem array of 5 units of 120 bases"""
    rng = np.random.default_rng(7301)
    G = rng.integers(0, 4, size=2 * CONTIG).astype(np.uint8)
    feats = []
    for i in range(N_FEAT):
        src, dst, kind = 2000 + SLOT * i, CONTIG + 2000 + SLOT * i, ("dup", "div3", "div4", "tandem")[i % 4]
        if kind == "tandem":
            for k in range(1, 5):
                G[src + 120 * k:src + 120 * (k + 1)] = G[src:src + 120]
        else:
            G[dst:dst + 300] = G[src:src + 300]
            if kind != "dup":
                at = dst + np.arange(12, 300, 34 if kind == "div3" else 25)
                G[at] = (G[at] + 1 + (at % 3)) & 3
        feats.append((kind, src, dst))
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    fa = b""
    for c in range(2):
        seq = acgt[G[c * CONTIG:(c + 1) * CONTIG]].tobytes()
        fa += b">c%d\n" % c + b"\n".join(seq[k:k + 80] for k in range(0, len(seq), 80)) + b"\n"
    return G, fa, feats


def pairing_reads(G, feats):
    rng = np.random.default_rng(7302)
    ins = lambda: int(np.clip(np.rint(rng.normal(400, 40)), 250, 550))   # noqa: E731
    reads = []
    for _ in range(200):   # ordinary pairs, for the statistics
        c = int(rng.integers(0, 2))
        reads += list(pair_reads(G, c * CONTIG + int(rng.integers(100, CONTIG - 700)), ins(), 1, 100))
    far = lambda k: CONTIG + 38_000 - 150 * k   # noqa: E731  (plain sequence at the end of c1)
    for rep in range(3):
        for i, (kind, src, dst) in enumerate(feats):
            n = ins()
            if kind == "tandem":     # mate 2 inside the array, mate 1 before it: candidate pairs 120 bases apart
                pos = src + 130 + 7 * rep + 100 - n
                reads += list(pair_reads(G, pos, n, 1, 100))
            elif kind == "dup":      # mate 2 inside the copy, mate 1 before it: two equal hits for mate 2
                pos = dst + 110 + 20 * rep + 100 - n
                reads += list(pair_reads(G, pos, n, 1, 100))
            else:                    # mate 2 is the source's sequence; the copy beside mate 1 has 3 or 4 substitutions
                off = 100 + 3 * rep
                m1, _ = pair_reads(G, dst + off + 100 - n, n, 1, 100)
                reads += [m1, rc(G[src + off:src + off + 100])]
            # a chimeric mate 1 (two primary regions) with a proper mate 2; and two unrelated ends
            k = 3 * i + rep
            pos = 300 + 450 * k % (CONTIG - 1000)
            m1, m2 = pair_reads(G, pos, n, 1, 100)
            if k % 2 == 0:
                reads += [np.concatenate([m1[:50], G[far(k):far(k) + 50]]), m2]
            else:
                reads += [m1, rc(G[far(k):far(k) + 100])]
    return reads


def write_set(name, man, fq, smrg, sam):
    for ext, data in ((".fq.gz", fq), (".smrg.gz", smrg)) + (((".sam.gz", sam),) if sam is not None else ()):
        with open(os.path.join(OUT, name + ext), "wb") as fh:
            fh.write(gzip.compress(data, 9, mtime=0))
    with open(os.path.join(OUT, name + ".json"), "w") as fh:
        json.dump(man, fh, indent=1)


def make_pairing_sets(only):
    from tests import matesw_data, pair_chain as PC
    G, fa, feats = make_p1()
    reads = pairing_reads(G, feats)
    l_pac, pac = int(G.size), matesw_data.pack(G)
    contigs = [("c0", 0, CONTIG), ("c1", CONTIG, CONTIG)]
    done = []
    for name, opts in (("rep", "default"), ("rep_a2", "a2")):
        if only and name not in only:
            continue
        fq, smrg, msg, sam = run_reference(fa, reads, True, a2=opts == "a2")
        rd, lists = PC.parse_set(fq, smrg)
        O = PC.OPTS[opts]
        fin, pes, out, status = PC.run_chain(G, l_pac, rd, lists, O)
        c = PC.counts(out, status)
        checked, left, bad = PC.compare_sam(sam, rd, fin, out, status, O, l_pac, pac, contigs)
        if bad:
            raise SystemExit(f"{name}: the restatement differs from the reference's SAM: {bad[:5]}")
        if len(left) > PC.MAX_HOST_FRACTION * len(out):
            raise SystemExit(f"{name}: {len(left)} of {len(out)} pairs are left to the host: {left[:10]}")
        short = {g: c[g] for g in PC.GROUPS if c[g] < PC.MIN_GROUP}
        if short:
            raise SystemExit(f"{name}: fewer than {PC.MIN_GROUP} pairs in {short} (all: {c})")
        man = dict(genome="p1", options=opts, pairs=len(out), read_len=100, pestat=msg, pairing=c,
                   left_to_host=[list(x) for x in left])
        done.append((name, man, fq, smrg, sam))
        print(name, c)
    if done:   # nothing is written unless every set passed
        with open(os.path.join(HERE, "p1.fa.gz"), "wb") as fh:
            fh.write(gzip.compress(fa, 9, mtime=0))
        for x in done:
            write_set(*x)


def main():
    if not oracle.ref_available():
        oracle.build(ref=True)
    from tests import golden_data, matesw_ref, pair_ref, regfin_ref
    os.makedirs(OUT, exist_ok=True)
    with gzip.open(os.path.join(HERE, "g1.fa.gz"), "rb") as fh:
        fa_bytes = fh.read()
    G = golden_data.fasta_codes(fa_bytes)
    l_pac = int(G.size)
    only = sys.argv[1:]
    for name, (reads, L) in sets(G).items():
        if only and name not in only:
            continue
        fq, smrg, msg, _ = run_reference(fa_bytes, reads, False)
        raw, raw_off = golden_data.smrg_parse(smrg)
        lists = [regfin_ref.sort_and_dedup([matesw_ref._as_dict(raw[k]) for k in range(int(raw_off[r]), int(raw_off[r + 1]))],
                                           0.95) for r in range(len(reads))]
        pes, n_cand, tr = pair_ref.pestat(pair_ref.Opt(), l_pac, lists)
        if not shows(name, msg, tr):
            raise SystemExit(f"{name}: the reference's messages do not show the case it was built for: {msg} {tr.sub_found} {tr.not_unique} {tr.sub_kept}")
        man = dict(genome="g1", pairs=len(reads) // 2, read_len=L, pestat=msg,
                   trace=dict(empty=tr.empty, not_unique=tr.not_unique, sub_found=tr.sub_found, sub_kept=tr.sub_kept, low_cap=tr.low_cap,
                              low1_clamp=tr.low1_clamp, low2_clamp=tr.low2_clamp))
        write_set(name, man, fq, smrg, None)
        print(name, msg["n_cand"], msg["few"], msg["ratio"], {d: v.get("bounds") for d, v in msg["dirs"].items()})
    make_pairing_sets(only)


if __name__ == "__main__":
    main()
