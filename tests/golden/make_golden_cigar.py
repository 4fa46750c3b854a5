"""Gapped-alignment fixtures for regions -> alignments (smem_reg2aln), from the
compiled reference alone (oracle/_ref/ref_harness).

    python tests/golden/make_golden_cigar.py

The other golden reads carry substitutions and Ns only, so their SAM holds
almost no gapped CIGAR.  For g1 and g2 this writes under tests/golden/cigar/:
  <g>.smrd.gz   ~370 reads made with synth._mutated_copy and a fixed seed (MIX
                below: substitutions, short indels, one longer insertion or
                deletion; half reverse-complemented, a fifth with one N)
  <g>.smrg.gz   the reference's regions of those reads (`ref_harness aln`:
                mem_chain2aln over its own seeds and chains, default options)
  <g>.tsv.gz    per mapped record of the reference's SAM (`ref_harness mem`,
                one thread, single-end): qname flag rname pos cigar NM MD
  manifest.json sha256 of each file's contents and the counts
A SAM record belongs to the region of its read with the record's geometry
(match_records); at most 2 % of the mapped records may find none.
"""
import gzip
import hashlib
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

from smemgpu import synth  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
OUT = os.path.join(HERE, "cigar")
# (count, (min, max) length, substitution rate, indel rate, (min, max) of one extra gap or None)
MIX = [
    (120, (100, 150), 0.02, 0.01, None),
    (120, (100, 150), 0.01, 0.02, (3, 12)),
    (60, (200, 400), 0.02, 0.015, (3, 30)),
    (40, (60, 100), 0.03, 0.03, None),
    (30, (150, 150), 0.0, 0.0, (3, 60)),
]
ALN_ARGS = ["19", "1.5", "10", "1", "10000", "100", "10000", "0.5", "0.5"]
MAX_UNMATCHED = 0.02


def make_reads(genome: np.ndarray, seed: int) -> synth.Reads:
    rng = np.random.default_rng(seed)
    parts = []
    for count, (lo, hi), sub, indel, gap in MIX:
        for _ in range(count):
            L = int(rng.integers(lo, hi + 1))
            p = int(rng.integers(0, genome.size - L - 64))
            src = genome[p:p + L]
            r = synth._mutated_copy(src, rng, sub, indel) if (sub or indel) else src.copy()
            if gap is not None:
                n = int(rng.integers(gap[0], gap[1] + 1))
                at = int(rng.integers(25, max(26, r.size - 25 - n)))
                if rng.random() < 0.5:   # insertion into the read
                    r = np.concatenate([r[:at], rng.integers(0, 4, size=n, dtype=np.uint8), r[at:]])
                else:                    # deletion from the read
                    r = np.concatenate([r[:at], r[at + n:]])
            if rng.random() < 0.5:
                r = (3 - r)[::-1]
            r = r.astype(np.uint8)
            if rng.random() < 0.2:
                r[int(rng.integers(0, r.size))] = 4
            parts.append(r)
    lens = np.array([p.size for p in parts], dtype=np.int32)
    return synth.Reads(lens, np.concatenate(parts), np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]))


def contigs(fa_gz: str) -> dict:
    """contig name -> (offset in the concatenated forward strand, length)"""
    out, name, off, n = {}, None, 0, 0
    with gzip.open(fa_gz, "rb") as fh:
        for line in fh:
            if line.startswith(b">"):
                if name is not None:
                    out[name] = (off, n)
                    off += n
                name, n = line[1:].split()[0].decode(), 0
            else:
                n += len(line.strip())
    out[name] = (off, n)
    return out


def sam_records(sam: bytes) -> list:
    """the mapped records as (qname, flag, rname, pos, cigar, NM, MD)"""
    out = []
    for line in sam.decode().split("\n"):
        if not line or line.startswith("@"):
            continue
        f = line.split("\t")
        if int(f[1]) & 4:
            continue
        tags = {t[:2]: t[5:] for t in f[11:]}
        out.append((f[0], int(f[1]), f[2], int(f[3]), f[5], int(tags["NM"]), tags["MD"]))
    return out


def parse_cigar(s: str) -> list:
    """SAM CIGAR -> [(op, len)] with op 0 M 1 I 2 D 3 S; a supplementary record's H
    is mem_aln2sam's print of the same clip (software/bwamem.c)"""
    return [("MIDSH".index(op) if op != "H" else 3, int(n)) for n, op in re.findall(r"(\d+)([MIDSH])", s)]


def match_records(records, regs, reg_off, lens, ctg, l_pac):
    """For each record the index of the region of its read (qname r<index>) with the
    same strand, clips, contig-relative position and reference length, or -1."""
    out = []
    for qname, flag, rname, pos, cigar, _nm, _md in records:
        r = int(qname[1:])
        ops = parse_cigar(cigar)
        rev = bool(flag & 16)
        c5 = ops[0][1] if ops[0][0] == 3 else 0
        c3 = ops[-1][1] if ops[-1][0] == 3 and len(ops) > 1 else 0
        rlen = sum(n for op, n in ops if op in (0, 2))
        gpos = ctg[rname][0] + pos - 1
        hit = -1
        for k in range(int(reg_off[r]), int(reg_off[r + 1])):
            g = regs[k]
            rb, re_, qb, qe = int(g["rb"]), int(g["re"]), int(g["qb"]), int(g["qe"])
            if rb < 0 or re_ < 0 or (rb < l_pac) == rev:
                continue
            L = int(lens[r])
            k5, k3 = (L - qe, qb) if rev else (qb, L - qe)
            if (k5, k3) == (c5, c3) and (2 * l_pac - re_ if rev else rb) == gpos and re_ - rb == rlen:
                hit = k
                break
        out.append(hit)
    return out


def main():
    import struct
    from tests import golden_data
    os.makedirs(OUT, exist_ok=True)
    man = {}
    with tempfile.TemporaryDirectory() as d:
        for g, seed in (("g1", 101), ("g2", 102)):
            fa_gz = os.path.join(HERE, g + ".fa.gz")
            fa = os.path.join(d, g + ".fa")
            with gzip.open(fa_gz, "rb") as src, open(fa, "wb") as dst:
                shutil.copyfileobj(src, dst)
            genome = golden_data.fasta_codes(open(fa, "rb").read())
            subprocess.run([REF, "index", fa, fa], check=True, capture_output=True)
            reads = make_reads(genome, seed)
            smrd, smrg, fq = (os.path.join(d, g + e) for e in (".smrd", ".smrg", ".fq"))
            synth.write_smrd(smrd, reads)
            synth.write_fastq(fq, reads)
            subprocess.run([REF, "aln", fa + ".bwt", fa + ".sa", fa + ".pac", smrd, smrg] + ALN_ARGS, check=True,
                           capture_output=True)
            sam = subprocess.run([REF, "mem", fa, fq, "1", "1", "0"], check=True, capture_output=True).stdout
            recs = sam_records(sam)
            tsv = "".join("\t".join(str(x) for x in r) + "\n" for r in recs).encode()
            blobs = {".smrd": open(smrd, "rb").read(), ".smrg": open(smrg, "rb").read(), ".tsv": tsv}
            for ext, data in blobs.items():
                with open(os.path.join(OUT, g + ext + ".gz"), "wb") as raw:
                    with gzip.GzipFile(fileobj=raw, mode="wb", compresslevel=9, mtime=0, filename="") as fh:
                        fh.write(data)
            regs, reg_off = golden_data.smrg_parse(blobs[".smrg"])
            l_pac = struct.unpack_from("<5Q", open(fa + ".bwt", "rb").read(), 0)[4] // 2
            hits = match_records(recs, regs, reg_off, reads.lens, contigs(fa_gz), l_pac)
            n_un = sum(1 for h in hits if h < 0)
            gapped = sum(1 for r, h in zip(recs, hits) if h >= 0 and re.search("[ID]", r[4]))
            assert n_un <= MAX_UNMATCHED * len(recs), (g, n_un, len(recs))
            man[g] = {"reads": int(reads.n), "regions": int(regs.size), "records": len(recs),
                      "matched": len(recs) - n_un, "matched_gapped": gapped,
                      "sha256": {ext[1:]: hashlib.sha256(data).hexdigest() for ext, data in blobs.items()}}
            print(g, man[g], flush=True)
    with open(os.path.join(OUT, "manifest.json"), "w") as fh:
        json.dump(man, fh, indent=1)


if __name__ == "__main__":
    main()
