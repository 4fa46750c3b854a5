"""Mate rescue restated (tests/matesw_ref.py) against the reference end to end.

Golden: tests/golden/msw (tests/golden/make_golden_msw.py --pairs-only), on g1:
250 ordinary pairs, from which the reference infers FR alone, and 60 pairs
whose second mate has a substitution at every tenth base -- no seed, no region
of its own.  The fixture holds the FASTQ, the reference's SAM (ref_harness mem),
its regions of every read before mem_sort_and_dedup (ref_harness aln) and the
bounds it printed.  The restatement gets the regions after
regfin_ref.sort_and_dedup and the recorded bounds; every read that had no region
must come out with exactly one, and reg2aln_ref.reg2aln of that region must give
the SAM line's strand, POS, CIGAR and NM (a read with a single region is printed
whatever pairing decides).

The hand-built pairs of tests/matesw_data.py are checked here for what each
group was built to reach; the GPU stage is compared with the restatement on both
in tests/test_gpu_matesw.py."""
import functools
import gzip
import json
import os

import numpy as np

from tests import golden_data, matesw_data as D, matesw_ref as R, reg2aln_ref, regfin_data, regfin_ref

MSW = os.path.join(golden_data.GOLDEN, "msw")


@functools.lru_cache(maxsize=None)
def load_set():
    """dict(G, pac, l_pac, pes, arrays = (codes, offs, regs, reg_off), sam = the primary record per read)"""
    from smemgpu import synth
    from smemgpu.lib import ALNREG_DT
    with open(os.path.join(MSW, "g1_pe.json")) as fh:
        man = json.load(fh)
    G = golden_data.fasta_codes(golden_data.gz("g1.fa.gz"))
    with gzip.open(os.path.join(MSW, "g1_pe.fq.gz"), "rb") as fh:
        lines = fh.read().split(b"\n")
    reads = [synth.NT4[np.frombuffer(lines[k + 1], dtype=np.uint8)].astype(np.uint8) for k in range(0, len(lines) - 1, 4)]
    assert len(reads) == 2 * man["pairs"]
    with gzip.open(os.path.join(MSW, "g1_pe.smrg.gz"), "rb") as fh:
        raw, raw_off = golden_data.smrg_parse(fh.read())
    lists = []
    for r in range(len(reads)):   # mem_align1_core ends with mem_sort_and_dedup (software/bwamem.c)
        a = [R._as_dict(raw[k]) for k in range(int(raw_off[r]), int(raw_off[r + 1]))]
        lists.append(regfin_ref.sort_and_dedup(a, 0.95))
    offs = np.concatenate([[0], np.cumsum([x.size for x in reads])]).astype(np.uint64)
    reg_off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    regs = np.zeros(int(reg_off[-1]), dtype=ALNREG_DT)
    k = 0
    for lst in lists:
        for x in lst:
            for f in regfin_ref.FIELDS:
                regs[k][f] = x[f]
            k += 1
    sam = {}
    with gzip.open(os.path.join(MSW, "g1_pe.sam.gz"), "rt") as fh:
        for line in fh:
            if line.startswith("@"):
                continue
            f = line.rstrip("\n").split("\t")
            flag = int(f[1])
            if flag & 0x900:
                continue
            nm = [int(t[5:]) for t in f[11:] if t.startswith("NM:i:")]
            sam[2 * int(f[0][1:]) + (1 if flag & 0x80 else 0)] = dict(flag=flag, rname=f[2], pos=int(f[3]), cigar=f[5],
                                                                     nm=nm[0] if nm else None)
    pes = [R.Pes(p["low"], p["high"], p["failed"]) for p in man["pes"]]
    return dict(G=G, pac=golden_data.pac("g1"), l_pac=golden_data.l_pac("g1"), pes=pes, reads=reads,
                arrays=(np.concatenate(reads), offs, regs, reg_off), sam=sam, man=man)


def test_msw_fixture_shape():
    S = load_set()
    codes, offs, regs, reg_off = S["arrays"]
    assert S["man"]["pairs"] == 310 and S["l_pac"] == S["G"].size
    assert [p.failed for p in S["pes"]] == [1, 0, 1, 1]            # the reference inferred FR alone
    assert 100 < S["pes"][1].low < 400 < 600 < S["pes"][1].high < 1000
    none = np.diff(reg_off.astype(np.int64)) == 0
    assert none.sum() >= 40 and (none[1::2].sum() == none.sum())    # the unseeded second mates
    assert all(not S["sam"][r]["flag"] & 4 for r in np.nonzero(none)[0])


def test_rescued_reads_match_the_reference_sam():
    S = load_set()
    codes, offs, regs, reg_off = S["arrays"]
    lists, n_sw, status, tr = R.matesw(R.Opt(), S["l_pac"], S["G"], S["pes"], codes, offs, regs, reg_off)
    assert not any(status)
    contigs = regfin_data.contigs("g1")
    none = np.nonzero(np.diff(reg_off.astype(np.int64)) == 0)[0]
    checked = 0
    for r in none:
        want = S["sam"][int(r)]
        assert not want["flag"] & 4
        assert len(lists[r]) == 1, f"read {r}: {len(lists[r])} regions after rescue"
        a = reg2aln_ref.reg2aln(reg2aln_ref.Opt(), S["l_pac"], S["pac"], S["reads"][r], lists[r][0])
        assert a.status == 0
        rname, pos = next((c, a.pos - off + 1) for c, off, n in contigs if off <= a.pos < off + n)
        got = (bool(a.is_rev), rname, pos, reg2aln_ref.cigar_str(a.cigar), a.NM)
        assert got == (bool(want["flag"] & 16), want["rname"], want["pos"], want["cigar"], want["nm"]), (int(r), got, want)
        checked += 1
    assert checked >= 40
    # the pairs that were consistent from the start are left alone
    quiet = [p for p in range(len(n_sw)) if tr[p].calls == 0]
    assert len(quiet) >= 200 and all(n_sw[p] == 0 for p in quiet)


def test_hand_built_pairs_reach_their_branches():
    G = D.genome()
    P = D.build(G)
    codes, offs, regs, reg_off = P.arrays()
    lists, n_sw, status, tr = R.matesw(R.Opt(), D.L_PAC, G, D.PES_ALL, codes, offs, regs, reg_off)
    for r, name in enumerate(("FF", "FR", "RF", "RR")):
        for p in P.of("rescue_" + name):
            assert (tr[p].sw, tr[p].inserted) == (4, 1)
            assert R.infer_dir(D.L_PAC, P.lists[2 * p][0]["rb"], lists[2 * p + 1][0]["rb"])[0] == r
    assert all(tr[p].clipped >= 2 for p in P.of("clip_0") + P.of("clip_2l"))
    assert all(tr[p].bridged == 2 and n_sw[p] == 2 for p in P.of("bridge"))
    assert all((tr[p].below, tr[p].inserted, n_sw[p]) == (4, 0, 4) for p in P.of("below"))
    assert all(tr[p].word == 4 for p in P.of("long250"))
    assert all([x["score"] for x in lists[2 * p + 1]] == [150] and tr[p].dedup_drop == 2 for p in P.of("dedup_drops_old"))
    assert all([x["score"] for x in lists[2 * p + 1]] == [200] and tr[p].dedup_drop == 2 for p in P.of("dedup_drops_new"))
    assert [p for p in range(len(status)) if status[p]] == P.of("host_300")
    P2 = D.build_fr(G)
    codes, offs, regs, reg_off = P2.arrays()
    lists, n_sw, status, tr = R.matesw(R.Opt(), D.L_PAC, G, D.PES_FR, codes, offs, regs, reg_off)
    assert all(tr[p].calls == 0 and n_sw[p] == 0 for p in P2.of("consistent"))
    assert all((tr[p].calls, tr[p].all_skipped, n_sw[p]) == (1, 1, 1) for p in P2.of("second_anchor_skips"))
    assert all((tr[p].calls, tr[p].sw, n_sw[p]) == (2, 2, 2) for p in P2.of("two_anchors"))


def test_infer_dir_table():
    """mem_infer_dir (software/bwamem_pair.c:23-30) on one point per orientation and strand"""
    L = 1000
    assert R.infer_dir(L, 100, 300) == (0, 200)              # FF
    assert R.infer_dir(L, 100, 2 * L - 1 - 300) == (1, 200)  # FR
    assert R.infer_dir(L, 300, 2 * L - 1 - 100) == (2, 200)  # RF
    assert R.infer_dir(L, 300, 100) == (3, 200)              # RR
    assert R.infer_dir(L, 2 * L - 1 - 300, 100) == (1, 200)  # a reverse anchor, the mate forward behind it
