"""Golden single-end SAM text for reads with split alignments (tests/test_samtext.py,
tests/test_gpu_samtext.py): what the unpatched reference pipeline prints for the r3 reads on
g1 and the r4 reads on g2, whose raw regions are already committed (g1_r3_default.smrg.gz,
g2_r4_default.smrg.gz).

    python tests/golden/make_golden_samtext.py

  samtext/g1_r3_default.sam.gz, samtext/g2_r4_default.sam.gz
      the whole output of `ref_harness mem` (-t 1 -b 1, single-end, default options) over a
      FASTQ of the set's reads of at least 30 bp, named and given qualities by
      tests/samtext_data.py (new_name, new_qual: names of varying length, qualities that are
      neither constant nor palindromic).  The FASTQ is not kept: the tests rebuild the names
      and qualities from the same rules.
  samtext/manifest.json   sha256 of each uncompressed file and what it holds

The committed single-end SAM (sam/g<n>_se.sam.gz) has one record per read, so no SA:Z, no
hard clip and one quality character; these sets have 111 / 60 supplementary records.  A file
must not exceed the largest golden file already committed (sam/g1_se.sam.gz); main() fails
rather than trim silently if one ever does.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from smemgpu import synth  # noqa: E402
import samtext_data  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
OUT = os.path.join(HERE, "samtext")
SETS = [("g1_r3_default", "g1", "r3.smrd.gz"), ("g2_r4_default", "g2", "r4.smrd.gz")]
MAX_BYTES = os.path.getsize(os.path.join(HERE, "sam", "g1_se.sam.gz"))


def write_fastq(path, reads, keep):
    acgtn = np.frombuffer(b"ACGTN", dtype=np.uint8)
    with open(path, "wb") as fh:
        for i in keep:
            s = acgtn[np.minimum(reads.read(int(i)), 4)].tobytes()
            q = samtext_data.new_qual(int(i), len(s)).tobytes()
            fh.write(b"@" + samtext_data.new_name(int(i)).encode() + b"\n" + s + b"\n+\n" + q + b"\n")


def main():
    os.makedirs(OUT, exist_ok=True)
    man = {}
    with tempfile.TemporaryDirectory() as d:
        for name, g, rfile in SETS:
            fa = os.path.join(d, g + ".fa")
            with gzip.open(os.path.join(HERE, g + ".fa.gz"), "rb") as src, open(fa, "wb") as dst:
                shutil.copyfileobj(src, dst)
            subprocess.run([REF, "index", fa, fa], check=True, capture_output=True)
            smrd = os.path.join(d, name + ".smrd")
            with gzip.open(os.path.join(HERE, rfile), "rb") as src, open(smrd, "wb") as dst:
                shutil.copyfileobj(src, dst)
            reads = synth.read_smrd(smrd)
            keep = np.nonzero(reads.lens >= samtext_data.MIN_LEN)[0]
            fq = os.path.join(d, name + ".fq")
            write_fastq(fq, reads, keep)
            sam = subprocess.run([REF, "mem", fa, fq, "1", "1", "0"], check=True, capture_output=True).stdout
            path = os.path.join(OUT, name + ".sam.gz")
            with open(path, "wb") as raw:
                with gzip.GzipFile(fileobj=raw, mode="wb", compresslevel=9, mtime=0, filename="") as fh:
                    fh.write(sam)
            if os.path.getsize(path) > MAX_BYTES:
                raise SystemExit(f"{path}: {os.path.getsize(path)} B exceeds {MAX_BYTES} B; select reads")
            lines = [l for l in sam.split(b"\n") if l and not l.startswith(b"@")]
            flags = [int(l.split(b"\t")[1]) for l in lines]
            man[name] = {"genome": g, "reads": rfile, "reads_kept": int(keep.size), "records": len(lines),
                         "supplementary": sum(1 for f in flags if f & 0x800), "unmapped": sum(1 for f in flags if f & 4),
                         "sha256": hashlib.sha256(sam).hexdigest()}
            print(name, man[name], os.path.getsize(path), flush=True)
    with open(os.path.join(OUT, "manifest.json"), "w") as fh:
        json.dump(man, fh, indent=1)


if __name__ == "__main__":
    main()
