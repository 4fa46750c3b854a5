"""Golden records for raw regions -> final regions (tests/test_regfin.py,
tests/test_gpu_regfin.py): what the unpatched reference pipeline prints for
reads whose raw regions are already committed.

    python tests/golden/make_golden_regfin.py

  regfin/cigar_g1.tsv.gz, regfin/cigar_g2.tsv.gz   the gapped reads of cigar/<g>.smrd.gz
  regfin/g2_r4.tsv.gz                              the committed r4 reads (g2, up to 700 bp)

One line per mapped record of `ref_harness mem` (-t 1 -b 1, single-end, reads
named r<index>; reads under 30 bp are left out as in make_golden_sam.py, so a
read's hash id is its ordinal among the reads kept): qname, flag, rname, pos,
MAPQ, AS, XS ("." when the reference prints none).  The cigar fixtures' own
.tsv has no MAPQ column; these files add it, and the long reads of r4 pin the
MAPQ cap of supplementary records.
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

REF = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
OUT = os.path.join(HERE, "regfin")
SETS = [("cigar_g1", "g1", os.path.join("cigar", "g1.smrd.gz")), ("cigar_g2", "g2", os.path.join("cigar", "g2.smrd.gz")),
        ("g2_r4", "g2", "r4.smrd.gz")]


def write_fastq(path, reads, keep):
    acgtn = np.frombuffer(b"ACGTN", dtype=np.uint8)
    with open(path, "wb") as fh:
        for i in keep:
            s = acgtn[np.minimum(reads.read(int(i)), 4)].tobytes()
            fh.write(b"@r%d\n" % int(i) + s + b"\n+\n" + b"I" * len(s) + b"\n")


def main():
    os.makedirs(OUT, exist_ok=True)
    man = {}
    with tempfile.TemporaryDirectory() as d:
        for g in ("g1", "g2"):
            fa = os.path.join(d, g + ".fa")
            with gzip.open(os.path.join(HERE, g + ".fa.gz"), "rb") as src, open(fa, "wb") as dst:
                shutil.copyfileobj(src, dst)
            subprocess.run([REF, "index", fa, fa], check=True, capture_output=True)
        for name, g, rfile in SETS:
            smrd = os.path.join(d, name + ".smrd")
            with gzip.open(os.path.join(HERE, rfile), "rb") as src, open(smrd, "wb") as dst:
                shutil.copyfileobj(src, dst)
            reads = synth.read_smrd(smrd)
            keep = np.nonzero(reads.lens >= 30)[0]
            fq = os.path.join(d, name + ".fq")
            write_fastq(fq, reads, keep)
            sam = subprocess.run([REF, "mem", os.path.join(d, g + ".fa"), fq, "1", "1", "0"], check=True,
                                 capture_output=True).stdout
            rows = []
            for line in sam.decode().split("\n"):
                if not line or line.startswith("@"):
                    continue
                f = line.split("\t")
                if int(f[1]) & 4:
                    continue
                tags = {t[:2]: t[5:] for t in f[11:] if t[:5] in ("AS:i:", "XS:i:")}
                rows.append("\t".join([f[0], f[1], f[2], f[3], f[4], tags.get("AS", "."), tags.get("XS", ".")]))
            data = ("\n".join(rows) + "\n").encode()
            with open(os.path.join(OUT, name + ".tsv.gz"), "wb") as raw:
                with gzip.GzipFile(fileobj=raw, mode="wb", compresslevel=9, mtime=0, filename="") as fh:
                    fh.write(data)
            man[name] = {"genome": g, "reads": rfile.replace(os.sep, "/"), "reads_kept": int(keep.size),
                         "records": len(rows), "sha256": hashlib.sha256(data).hexdigest()}
            print(name, man[name], flush=True)
    with open(os.path.join(OUT, "manifest.json"), "w") as fh:
        json.dump(man, fh, indent=1)


if __name__ == "__main__":
    main()
