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
group was built to reach, and against the reference's own mem_matesw on the same
lists (tests/golden/msw/hand, make_golden_msw.py --hand-only: ref_harness msw):
every field of every region in order and the returned n, for every pair the
restatement does not leave to the host.  The GPU stage is compared with the
restatement and with those files in tests/test_gpu_matesw.py."""
import functools
import gzip
import json
import os

import numpy as np
import pytest

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


# ---- the reference's own mem_matesw on the hand-built pairs (tests/golden/msw/hand) -----------
HAND = os.path.join(MSW, "hand")
with open(os.path.join(HAND, "manifest.json")) as _fh:
    MANIFEST = json.load(_fh)


@functools.lru_cache(maxsize=None)
def hand_batches():
    return D.fixtures()


@functools.lru_cache(maxsize=None)
def hand(name):
    """(G, l_pac, Case, the batch's arrays, the reference's (regs, reg_off, n), the restatement's result)"""
    import hashlib
    G, l_pac, case = hand_batches()[name]
    man = MANIFEST[name]
    assert hashlib.sha256(D.smmi_bytes(G, l_pac, case)).hexdigest() == man["input_sha256"], \
        f"{name}: the builder no longer gives what the fixture was recorded from"
    assert man["pairs"] == len(case.pairs.group) and man["l_pac"] == l_pac
    with gzip.open(os.path.join(HAND, name + ".smmo.gz"), "rb") as fh:
        ref = D.smmo_parse(fh.read())
    arrays = case.pairs.arrays()
    return G, l_pac, case, arrays, ref, R.matesw(case.opt, l_pac, G, case.pes, *arrays)


def ref_lists(ref, p):
    regs, reg_off, n = ref
    return [[R._as_dict(regs[k]) for k in range(int(reg_off[2 * p + e]), int(reg_off[2 * p + e + 1]))] for e in range(2)]


def test_hand_fixture_list():
    assert sorted(MANIFEST) == sorted(hand_batches())
    for o in D.OPTS:
        assert MANIFEST[f"all_{o}"]["builder"] == "build" and MANIFEST[f"fr_{o}"]["builder"] == "build_fr"
    edges = D.build_edges(D.genome(), D.L_PAC)
    assert set(edges) == set(D.EDGE_SIZES)
    for name, c in edges.items():
        assert {g: len(c.pairs.of(g)) for g in dict.fromkeys(c.pairs.group)} == D.EDGE_SIZES[name], name
        assert 2 <= len(c.pairs.group) <= 12


@pytest.mark.parametrize("name", sorted(MANIFEST))
def test_restatement_equals_the_reference(name):
    """every pair the restatement keeps: its lists equal the reference's mem_matesw loop field by field and in
    order, and so is n; every pair it leaves to the host: for a reason it names, and the reference did
    something there"""
    G, l_pac, case, (codes, offs, regs, reg_off), ref, (lists, n_sw, status, tr) = hand(name)
    assert ref[2].size == len(status)
    kept = 0
    for p in range(len(status)):
        want = ref_lists(ref, p)
        if status[p] == 0:
            kept += 1
            assert n_sw[p] == int(ref[2][p]), (name, p, case.pairs.group[p], n_sw[p], int(ref[2][p]))
            for e in range(2):
                got = lists[2 * p + e]
                assert len(got) == len(want[e]), (name, p, e, case.pairs.group[p], len(got), len(want[e]))
                for k, (x, y) in enumerate(zip(got, want[e])):
                    assert x == y, (name, p, e, k, case.pairs.group[p], x, y)
        else:
            assert tr[p].host in ("mate", "window", "list")
            lens = [int(offs[2 * p + e + 1] - offs[2 * p + e]) for e in range(2)]
            if tr[p].host == "mate":
                assert max(lens) > 256 or min(lens) < 1
            before = [[R._as_dict(regs[k]) for k in range(int(reg_off[2 * p + e]), int(reg_off[2 * p + e + 1]))]
                      for e in range(2)]
            # (with max_matesw = 0 nobody does anything: the mate's length sends the pair off before any anchor counts)
            assert int(ref[2][p]) > 0 or want != before or case.opt.max_matesw == 0, (name, p, "the reference did nothing here")
            assert lists[2 * p] == before[0] and lists[2 * p + 1] == before[1] and n_sw[p] == 0
    assert kept > 0 or name.startswith("roll_")


def test_edges_reach_their_branches():
    l_pac = D.L_PAC
    # long lists
    G, _, case, arrays, ref, (lists, n_sw, status, tr) = hand("long_base")
    P = case.pairs
    for n in D.LONG_SIZES[:-1]:
        (p,) = P.of(f"long_{n}")
        before = P.lists[2 * p + 1]
        (at, had), = tr[p].at
        assert status[p] == 0 and had == n == len(before) and tr[p].inserted == 1
        assert before[at - 1]["score"] == 150 == before[at - 2]["score"]       # inside a run of equals
        assert at == n or before[at]["score"] < 150
        assert n < 65 or at >= 64                        # not found by the first 64 lanes
        assert n < 128 or n // 64 > at // 64             # the copy shifts elements across a 64-boundary
        assert tr[p].dedup_drop == (n // 8 if n < 1000 else 0)
        assert len(lists[2 * p + 1]) == n + 1 - tr[p].dedup_drop
    assert len(lists[2 * P.of("long_1023")[0] + 1]) == R.MAX_REGS
    (p,) = P.of("long_1024_host")
    assert status[p] == R.MSW_HOST and tr[p].host == "list" and tr[p].inserted == 0
    (p,) = P.of("two_1022")
    assert status[p] == 0 and tr[p].inserted == 2 and tr[p].dedup_drop == 0 and len(lists[2 * p + 1]) == R.MAX_REGS
    (p,) = P.of("two_1023_host")
    assert status[p] == R.MSW_HOST and tr[p].host == "list" and tr[p].inserted == 1    # rolled back after an insertion
    (p,) = P.of("two_1023_twin")
    assert status[p] == 0 and tr[p].inserted == 2 and tr[p].dedup_drop == 1 and len(lists[2 * p + 1]) == R.MAX_REGS
    # roll-back
    G, _, case, arrays, ref, (lists, n_sw, status, tr) = hand("roll_base")
    P = case.pairs
    assert all(st == R.MSW_HOST and t.host == "window" for st, t in zip(status, tr))
    assert all((tr[p].inserted, tr[p].sw, tr[p].calls) == (1, 1, 1) and len(P.lists[2 * p + 1]) == 1 for p in P.of("roll_window"))
    assert all((tr[p].inserted, tr[p].sw, tr[p].calls) == (1, 2, 2) for p in P.of("roll_second"))
    # both ends
    G, _, case, arrays, ref, (lists, n_sw, status, tr) = hand("both_base")
    for p in case.pairs.of("both"):
        assert (status[p], n_sw[p], tr[p].inserted) == (0, 2, 2) and len(lists[2 * p]) == 2 and len(lists[2 * p + 1]) == 2
    # mates with N
    G, _, case, arrays, ref, (lists, n_sw, status, tr) = hand("n_base")
    P = case.pairs
    for n in (1, 5, 30):
        for r, o in enumerate(("FF", "FR")):
            (p,) = P.of(f"n_{n}_{o}")
            ms = P.reads[2 * p + 1]
            assert int((ms == 4).sum()) == n and (ms[0] == 4 or ms[-1] == 4) and (n == 1 or ms[0] == 4 == ms[-1])
            assert (status[p], tr[p].sw, tr[p].inserted) == (0, 4, 1)
            assert R.infer_dir(l_pac, P.lists[2 * p][0]["rb"], lists[2 * p + 1][0]["rb"])[0] == r
    assert P.reads[2 * P.of("n_1_FF")[0] + 1][0] == 4 and P.reads[2 * P.of("n_1_FR")[0] + 1][-1] == 4
    # l_pac, whatever it leaves modulo 4
    for name in ["lpac_base"] + [f"lpac{l}_base" for l in D.L_PAC_ODD]:
        G, l, case, arrays, ref, (lists, n_sw, status, tr) = hand(name)
        assert l == G.size and (name == "lpac_base" or l % 4)
        P = case.pairs
        at = {g: P.of(g)[0] for g in D.EDGE_SIZES["lpac"]}
        assert not any(status)
        p = at["ends_at_l_pac"]
        assert any(w[0] == 1 and w[2] == l for w in tr[p].windows) and tr[p].inserted == 1 and tr[p].bridged >= 1
        assert (lists[2 * p + 1][0]["rb"], lists[2 * p + 1][0]["score"]) == (l, 150)
        p = at["starts_at_l_pac"]
        assert any(w[0] == 3 and w[1] == l for w in tr[p].windows) and tr[p].inserted == 1
        assert (lists[2 * p + 1][0]["rb"], lists[2 * p + 1][0]["score"]) == (l, 150)
        p = at["starts_at_l_pac_fr"]
        assert any(w[0] == 1 and w[1] == l for w in tr[p].windows) and tr[p].inserted == 1
        assert (lists[2 * p + 1][0]["rb"], lists[2 * p + 1][0]["score"]) == (l - 150, 150)
        p = at["ends_past_l_pac"]
        assert any(w[0] == 1 and w[1] < l and w[2] == l + 1 for w in tr[p].windows)
        assert (tr[p].bridged, tr[p].inserted, n_sw[p]) == (2, 0, 2)
        p = at["clip_2l"]
        assert any(w[0] == 1 and w[2] == 2 * l for w in tr[p].windows) and tr[p].clipped >= 1 and tr[p].inserted == 1
        assert (lists[2 * p + 1][0]["rb"], lists[2 * p + 1][0]["score"]) == (0, 150)
    # window length
    G, _, case, arrays, ref, (lists, n_sw, status, tr) = hand("window_base")
    P = case.pairs
    for p in P.of("win_2048"):
        (w,) = tr[p].windows
        assert w[2] - w[1] == R.MAX_TLEN and (status[p], tr[p].inserted, tr[p].clipped) == (0, 1, 0)
    for p in P.of("win_2049"):
        (w,) = tr[p].windows
        assert w[2] - w[1] == R.MAX_TLEN + 1 and status[p] == R.MSW_HOST and tr[p].host == "window"
    for p in P.of("win_clip0"):
        (w,) = tr[p].windows
        assert w[1] == 0 and w[2] <= R.MAX_TLEN and P.reads[2 * p + 1].size + 1898 == 2100
        assert (status[p], tr[p].inserted, tr[p].clipped, tr[p].byte) == (0, 1, 1, 1)
    # equal scores
    G, _, case, arrays, ref, (lists, n_sw, status, tr) = hand("equal_base")
    for p in case.pairs.of("equal"):
        had = len(case.pairs.lists[2 * p + 1])
        assert tr[p].at == [(2, had)] and status[p] == 0
        after = lists[2 * p + 1]
        assert [x["score"] for x in after[:3]] == [150] * 3 and len(after) == had + 1
        assert after[0]["rb"] < after[1]["rb"] < l_pac <= after[2]["rb"] and after[2]["secondary"] == -1
    # short mates
    G, _, case, arrays, ref, (lists, n_sw, status, tr) = hand("short_base")
    P = case.pairs
    want = {1: (1, 0, 1, 0), 18: (1, 0, 1, 0), 19: (0, 1, 1, 0), 20: (0, 1, 1, 0), 249: (0, 1, 1, 0), 250: (0, 1, 0, 1),
            256: (0, 1, 0, 1)}
    assert tuple(want) == D.SHORT_SIZES
    for n, w in want.items():
        (p,) = P.of(f"short_{n}")
        assert P.reads[2 * p + 1].size == n and status[p] == 0 and n_sw[p] == 1
        assert (tr[p].below, tr[p].inserted, tr[p].byte, tr[p].word) == w, (n, tr[p])


def test_infer_dir_table():
    """mem_infer_dir (software/bwamem_pair.c:23-30) on one point per orientation and strand"""
    L = 1000
    assert R.infer_dir(L, 100, 300) == (0, 200)              # FF
    assert R.infer_dir(L, 100, 2 * L - 1 - 300) == (1, 200)  # FR
    assert R.infer_dir(L, 300, 2 * L - 1 - 100) == (2, 200)  # RF
    assert R.infer_dir(L, 300, 100) == (3, 200)              # RR
    assert R.infer_dir(L, 2 * L - 1 - 300, 100) == (1, 200)  # a reverse anchor, the mate forward behind it
