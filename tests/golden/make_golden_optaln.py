"""The reference's records for the r3 / r4 reads under the option sets whose raw
regions are already committed (tests/golden/<g>_<rs>_<oname>.smrg.gz), for
tests/test_optaln.py and tests/test_gpu_optaln.py: raw regions -> final regions
and regions -> alignments on reads of up to 1 kbp, under non-default scoring,
bands and seed lengths.

    python tests/golden/make_golden_optaln.py

  optaln/<g>_<rs>_<oname>.tsv.gz   (r3, g1) and (r4, g2) x SETS
  optaln/manifest.json             per file: sha256 of the contents, read set, genome, the
                                   full option dict, reads kept, records, records matched to a
                                   region of the committed .smrg, matched records with a gap

One line per mapped record of `ref_harness mem` (-t 1 -b 1, single-end, reads
named r<index>; reads under 30 bp are left out as in make_golden_regfin.py, so
a read's hash id is its ordinal among the reads kept): qname, flag, rname, pos,
MAPQ, CIGAR, NM, MD, AS, XS ("." when the reference prints no such tag).  All
eight options are given (-k -w -A -B -O d,i -E d,i -L 5,3 -d), so -A scales
nothing but T and pen_unpaired.  Uses the compiled reference only
(oracle/_ref/ref_harness).
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
sys.path.insert(0, HERE)

from smemgpu import synth  # noqa: E402
from make_golden_cigar import contigs, match_records  # noqa: E402
from make_golden_regfin import write_fastq  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
OUT = os.path.join(HERE, "optaln")
READS = [("g1", "r3"), ("g2", "r4")]
SETS = ["default", "gaps", "A3", "A100", "B1", "B9", "w1", "w7", "k10"]


def option_args(o):
    return ["-k", str(o["min_seed_len"]), "-w", str(o["w"]), "-A", str(o["a"]), "-B", str(o["b"]),
            "-O", f"{o['o_del']},{o['o_ins']}", "-E", f"{o['e_del']},{o['e_ins']}",
            "-L", f"{o['pen_clip5']},{o['pen_clip3']}", "-d", str(o["zdrop"])]


def sam_rows(sam: bytes):
    rows = []
    for line in sam.decode().split("\n"):
        if not line or line.startswith("@"):
            continue
        f = line.split("\t")
        if int(f[1]) & 4:
            continue
        tags = {t[:2]: t[5:] for t in f[11:]}
        rows.append([f[0], f[1], f[2], f[3], f[4], f[5], tags.get("NM", "."), tags.get("MD", "."), tags.get("AS", "."),
                     tags.get("XS", ".")])
    return rows


def main():
    from tests import aln_reads, golden_data
    os.makedirs(OUT, exist_ok=True)
    fixtures = {f["file"]: f for f in golden_data.aln_fixtures()}
    man = {}
    with tempfile.TemporaryDirectory() as d:
        for g, rs in READS:
            fa = os.path.join(d, g + ".fa")
            with gzip.open(os.path.join(HERE, g + ".fa.gz"), "rb") as src, open(fa, "wb") as dst:
                shutil.copyfileobj(src, dst)
            subprocess.run([REF, "index", fa, fa], check=True, capture_output=True)
            ctg = contigs(os.path.join(HERE, g + ".fa.gz"))
            l_pac = golden_data.l_pac(g)
            smrd = os.path.join(d, rs + ".smrd")
            with gzip.open(os.path.join(HERE, rs + ".smrd.gz"), "rb") as src, open(smrd, "wb") as dst:
                shutil.copyfileobj(src, dst)
            all_reads = synth.read_smrd(smrd)
            for oname in SETS:
                name = f"{g}_{rs}_{oname}"
                fix = fixtures[name + ".smrg.gz"]
                o = aln_reads.full_options(oname)
                assert fix["opt"] == o
                reads = all_reads.subset(np.arange(fix["n_reads"]))
                keep = np.nonzero(reads.lens >= 30)[0]
                fq = os.path.join(d, name + ".fq")
                write_fastq(fq, reads, keep)
                sam = subprocess.run([REF, "mem", fa, fq, "1", "1", "0", "@PG\tID:bwa\tPN:bwa"] + option_args(o),
                                     check=True, capture_output=True).stdout
                rows = sam_rows(sam)
                data = "".join("\t".join(r) + "\n" for r in rows).encode()
                with open(os.path.join(OUT, name + ".tsv.gz"), "wb") as raw:
                    with gzip.GzipFile(fileobj=raw, mode="wb", compresslevel=9, mtime=0, filename="") as fh:
                        fh.write(data)
                regs, reg_off = golden_data.smrg_parse(golden_data.smrg(fix))
                recs = [(r[0], int(r[1]), r[2], int(r[3]), r[5], r[6], r[7]) for r in rows]
                hits = match_records(recs, regs, reg_off, reads.lens, ctg, l_pac)
                man[name] = {"genome": g, "reads": rs, "n_reads": int(reads.n), "opt": o, "reads_kept": int(keep.size),
                             "records": len(rows), "matched": sum(1 for h in hits if h >= 0),
                             "matched_gapped": sum(1 for r, h in zip(recs, hits) if h >= 0 and re.search("[ID]", r[4])),
                             "sha256": hashlib.sha256(data).hexdigest()}
                print(name, {k: v for k, v in man[name].items() if k not in ("opt", "sha256")}, flush=True)
    with open(os.path.join(OUT, "manifest.json"), "w") as fh:
        json.dump(man, fh, indent=1)


if __name__ == "__main__":
    main()
