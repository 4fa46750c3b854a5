"""The restated paired-end pipeline over a set of tests/golden/pair, shared by
tests/test_pair.py, tests/test_gpu_pair.py and tests/golden/make_golden_pair.py:

    the reference's regions -> regfin_ref.sort_and_dedup -> pair_ref.pestat -> matesw_ref.matesw
    -> regfin_ref.mark_primary_se(id << 1 | end) -> pair_ref.pair -> reg2aln_ref.reg2aln

and its comparison with the reference's SAM: FLAG & 2, strand, RNAME / POS, MAPQ and XS of both
primary lines of every pair.  Option sets: "default" is mem_opt_init, "a2" what `-A 2` makes of
it (software/fastmap.c:111-120: b, the gap penalties, T, zdrop, the clip penalties and
pen_unpaired all scaled by a).
"""
import gzip
import json
import os
from collections import Counter

import numpy as np

from tests import golden_data, matesw_data, matesw_ref, pair_ref, reg2aln_ref, regfin_data, regfin_ref

PAIR = os.path.join(golden_data.GOLDEN, "pair")
_SC2 = dict(a=2, b=8, o_del=12, e_del=2, o_ins=12, e_ins=2)
OPTS = {
    "default": dict(pair=pair_ref.Opt(), msw=matesw_ref.Opt(), fin=regfin_ref.Opt(), g2a=reg2aln_ref.Opt()),
    "a2": dict(pair=pair_ref.Opt(pen_unpaired=34, T=60, **_SC2), msw=matesw_ref.Opt(pen_unpaired=34, **_SC2),
               fin=regfin_ref.Opt(T=60, **_SC2), g2a=reg2aln_ref.Opt(**_SC2)),
}
# the groups a pairing set must reach, ten pairs each (a tie decided by the hash is wanted too; its count is recorded)
GROUPS = ("branch0_multi", "branch0_none", "branch1_z_not_00", "branch1_mapq_raised", "branch2", "n_sub_above_0")
MIN_GROUP = 10
MAX_HOST_FRACTION = 0.02


def genome(name):
    """(codes, l_pac, 2-bit pac, contigs) of tests/golden/<name>.fa.gz"""
    G = golden_data.fasta_codes(golden_data.gz(name + ".fa.gz"))
    return G, int(G.size), matesw_data.pack(G), regfin_data.contigs(name)


def parse_set(fq_bytes, smrg_bytes):
    """(reads, each read's list after mem_sort_and_dedup) from a set's FASTQ and SMRG bytes"""
    from smemgpu import synth
    lines = fq_bytes.split(b"\n")
    reads = [synth.NT4[np.frombuffer(lines[k + 1], dtype=np.uint8)].astype(np.uint8) for k in range(0, len(lines) - 1, 4)]
    raw, raw_off = golden_data.smrg_parse(smrg_bytes)
    assert raw_off.size - 1 == len(reads)
    lists = [regfin_ref.sort_and_dedup([matesw_ref._as_dict(raw[k]) for k in range(int(raw_off[r]), int(raw_off[r + 1]))], 0.95)
             for r in range(len(reads))]
    return reads, lists


def load_set(name):
    """(manifest, reads, lists, SAM bytes or None) of a committed set"""
    with open(os.path.join(PAIR, name + ".json")) as fh:
        man = json.load(fh)
    with gzip.open(os.path.join(PAIR, name + ".fq.gz"), "rb") as fh:
        fq = fh.read()
    with gzip.open(os.path.join(PAIR, name + ".smrg.gz"), "rb") as fh:
        smrg = fh.read()
    reads, lists = parse_set(fq, smrg)
    assert len(reads) == 2 * man["pairs"]
    sam = None
    if os.path.exists(os.path.join(PAIR, name + ".sam.gz")):
        with gzip.open(os.path.join(PAIR, name + ".sam.gz"), "rb") as fh:
            sam = fh.read()
    return man, reads, lists, sam


def run_chain(G, l_pac, reads, lists, O):
    """(lists after rescue and mem_mark_primary_se, pes, [(sel, Trace)] per pair, rescue status per pair)"""
    pes, _, _ = pair_ref.pestat(O["pair"], l_pac, lists)
    offs = np.concatenate([[0], np.cumsum([x.size for x in reads])]).astype(np.uint64)
    reg_off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    flat = [x for lst in lists for x in lst]
    after, _, status, _ = matesw_ref.matesw(O["msw"], l_pac, G, pes, np.concatenate(reads), offs, flat, reg_off)
    fin = [regfin_ref.mark_primary_se(O["fin"], after[r], (r >> 1) << 1 | (r & 1)) for r in range(len(reads))]
    out = [pair_ref.pair(O["pair"], l_pac, pes, (fin[2 * p], fin[2 * p + 1]), p) for p in range(len(reads) // 2)]
    return fin, pes, out, status


def counts(out, status):
    """pairs per group of GROUPS, per branch, left to the host, and ties decided by the hash"""
    c = Counter({g: 0 for g in GROUPS})
    for p, (sel, t) in enumerate(out):
        if sel["status"] or status[p]:
            c["host"] += 1
            continue
        c[f"branch{sel['branch']}"] += 1
        if sel["branch"] == 0:
            c["branch0_" + t.why0] += 1
        c["branch1_z_not_00"] += sel["branch"] == 1 and sel["z"] != [0, 0]
        c["branch1_mapq_raised"] += sel["branch"] == 1 and bool(t.raised)
        c["n_sub_above_0"] += sel["n_sub"] > 0
        c["tie_by_hash"] += bool(t.tie)
    return {k: int(v) for k, v in sorted(c.items())}


def compare_sam(sam_bytes, reads, fin, out, status, O, l_pac, pac, contigs):
    """every pair the restatement keeps against both primary lines of the reference's SAM; returns
    (pairs checked, [(pair, reason)] left to the host, [mismatches])"""
    sam = {}
    for line in sam_bytes.decode().split("\n"):
        f = line.split("\t")
        if not line or line.startswith("@") or int(f[1]) & 0x900:
            continue
        xs = [int(t[5:]) for t in f[11:] if t.startswith("XS:i:")]
        sam[2 * int(f[0][1:]) + (1 if int(f[1]) & 0x80 else 0)] = (int(f[1]), f[2], int(f[3]), int(f[4]), xs[0] if xs else None)
    left, bad, checked = [], [], 0
    for p, (sel, tr) in enumerate(out):
        if sel["status"] or status[p]:
            left.append((p, tr.host or "rescue"))
            continue
        got = []
        for e in range(2):
            a = fin[2 * p + e]
            if sel["branch"] == 0:   # the single-end selection has the first record's MAPQ and XS
                if not a or a[0]["score"] < O["fin"].T:
                    got.append(None)
                    continue
                sse, _ = regfin_ref.select(O["fin"], a)
                reg, mapq, xs = a[0], sse[0][0], sse[0][2]
            else:
                reg = dict(a[sel["z"][e]])
                if sel["branch"] == 1:
                    reg["sub"] = sel["sub"][e]    # line 291
                mapq, xs = sel["mapq"][e], max(reg["sub"], reg["csub"])
            al = reg2aln_ref.reg2aln(O["g2a"], l_pac, pac, reads[2 * p + e], reg)
            if al.status != 0:
                bad.append((p, e, "no alignment"))
                got.append(None)
                continue
            rname, pos = next((c, al.pos - off + 1) for c, off, n in contigs if off <= al.pos < off + n)
            got.append((bool(al.is_rev), rname, pos, mapq, xs))
        same = got[0] is not None and got[1] is not None and got[0][1] == got[1][1]   # h[0].rid == h[1].rid >= 0 (:321)
        proper = 2 if sel["proper"] and (sel["branch"] or same) else 0
        for e in range(2):
            flag, rname, pos, mapq, xs = sam[2 * p + e]
            if got[e] is None:
                if not flag & 4:
                    bad.append((p, e, "mapped in the reference", sam[2 * p + e]))
            elif (flag & 2, bool(flag & 16), rname, pos, mapq, xs) != (proper,) + got[e]:
                bad.append((p, e, sel, sam[2 * p + e], (proper,) + got[e]))
        checked += 1
    return checked, left, bad
