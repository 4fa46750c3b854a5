"""Fixtures shared by tests/test_samtext.py and tests/test_gpu_samtext.py: read names,
qualities and the reference's SAM lines of four read sets whose raw regions are committed,
and the restatement's text of every read (tests/samtext_ref.py over tests/regfin_ref.py,
tests/reg2aln_ref.py and tests/xref_ref.py).

  g1_default_std, g2_default_std   the golden single-end reads: names r<i>, one constant quality,
                                   lines of sam/g<n>_se.sam.gz
  g1_r3_default, g2_r4_default     the r3 / r4 reads (up to ~700 bp, split alignments): names and
                                   qualities by the rules below, lines of samtext/<set>.sam.gz
                                   (tests/golden/make_golden_samtext.py)
"""
import functools
import gzip
import hashlib
import json
import os

import numpy as np

import regfin_ref
import samtext_ref as S
import xref_ref as X
from tests import golden_data

NEW_SETS = ("g1_r3_default", "g2_r4_default")
OLD_SETS = ("g1_default_std", "g2_default_std")
SETS = OLD_SETS + NEW_SETS
MIN_LEN = 30          # the reference's FASTQ leaves shorter reads out (tests/golden/make_golden_sam.py)


def new_name(i):
    """read i's name in the new fixtures: 2 to 21 bytes, the index first"""
    return f"r{i}" + (":" + "abcdefghijklmnopq"[:i % 17] if i % 3 else "")


def new_qual(i, n):
    """read i's qualities in the new fixtures: neither constant nor palindromic"""
    return (33 + (7 * i + 3 * np.arange(n)) % 41).astype(np.uint8)


def _fix(name):
    return next(f for f in golden_data.aln_fixtures() if f["file"] == name + ".smrg.gz")


def _golden_lines(name):
    """{read index: [line bytes with the newline, ...]} of the reference's SAM"""
    if name in NEW_SETS:
        d = os.path.join(golden_data.GOLDEN, "samtext")
        with open(os.path.join(d, "manifest.json")) as fh:
            man = json.load(fh)[name]
        with gzip.open(os.path.join(d, name + ".sam.gz"), "rb") as fh:
            data = fh.read()
        assert hashlib.sha256(data).hexdigest() == man["sha256"], "fixture corrupted"
    else:
        with gzip.open(os.path.join(golden_data.GOLDEN, "sam", name[:2] + "_se.sam.gz"), "rb") as fh:
            data = fh.read()
    out = {}
    for line in data.split(b"\n"):
        if line and not line.startswith(b"@"):
            qname = line.split(b"\t", 1)[0].decode()
            out.setdefault(int(qname.split(":")[0][1:]), []).append(line + b"\n")
    return out


@functools.lru_cache(maxsize=None)
def load(name):
    """dict(g, reads, names, quals (one uint8 array over all reads, the reads' offsets), regs,
    reg_off, lens, ids, l_pac, contigs, golden): golden[r] the reference's lines of read r
    joined, None for a read the reference never saw (under MIN_LEN)"""
    import regfin_data as D
    fix = _fix(name)
    g = fix["genome"]
    reads = golden_data.aln_reads(fix)
    regs, reg_off = golden_data.smrg_parse(golden_data.smrg(fix))
    lens = reads.lens.astype(np.int32)
    assert reg_off.size == lens.size + 1
    ids = np.cumsum(lens >= MIN_LEN).astype(np.int64) - 1
    if name in NEW_SETS:
        names = [new_name(i) for i in range(lens.size)]
        quals = np.concatenate([new_qual(i, int(n)) for i, n in enumerate(lens)])
    else:
        names = [f"r{i}" for i in range(lens.size)]
        quals = np.full(int(lens.sum()), 33 + 40, dtype=np.uint8)
    lines = _golden_lines(name)
    golden = [b"".join(lines[r]) if lens[r] >= MIN_LEN else None for r in range(lens.size)]
    assert all(r < lens.size and lens[r] >= MIN_LEN for r in lines)
    return dict(g=g, reads=reads, names=names, quals=quals, regs=regs, reg_off=reg_off, lens=lens, ids=ids,
                l_pac=golden_data.l_pac(g), contigs=D.contigs(g), golden=golden)


@functools.lru_cache(maxsize=None)
def records(name):
    """per read the samtext_ref.Rec list of the restatements at the default options"""
    F = load(name)
    opt = regfin_ref.Opt()
    fin = [regfin_ref.finalize(opt, F["regs"][int(F["reg_off"][r]):int(F["reg_off"][r + 1])], int(F["lens"][r]),
                               int(F["ids"][r])) for r in range(F["lens"].size)]
    rows = X.expected_rows(X.aligned_rows(fin, F["l_pac"], golden_data.pac(F["g"]), F["reads"]), F["contigs"],
                           F["l_pac"])
    return [S.recs_of(row, a, sel) for row, (a, sel, _idx) in zip(rows, fin)]


def qual_of(F, r):
    o = int(F["reads"].offs[r])
    return F["quals"][o:o + int(F["lens"][r])]


@functools.lru_cache(maxsize=None)
def texts(name):
    """per read the restatement's text, None for a read left to the host"""
    F = load(name)
    ctg_names, ctg_offs, _lens = X.table(F["contigs"])
    return [S.read_text(F["names"][r], F["reads"].read(r), qual_of(F, r), None, ctg_names, ctg_offs, recs)
            for r, recs in enumerate(records(name))]


# what the restatement leaves to the host (SMEM_ALN_XREF records), measured once and pinned here:
# the GPU stage must mark exactly these reads
HOST_READS = {"g1_r3_default": [78, 110], "g2_r4_default": [157]}
HOST_CAP = 0.01       # a set with more than 1 % of its reads left out checks too little

