"""ksw_align2 (software/ksw.c:342-364, ksw_u8 / ksw_i16 :110-333): the local SW
of mem_chain2aln_short (software/bwamem.c:805-852).

Golden: tests/golden/kswa_*.smat/.smar, the compiled reference's own
ksw_align2 (tests/golden/make_golden.py --kswa-only):
  kswa_a1, kswa_a2   3000 problems each, shaped like the short path (query span
                     of the seeds + 50 each side, < 200 bp, against the
                     reference span + 50), under mem_opt_init's scoring (a = 1:
                     every problem byte-scored) and -A 2 scaling (a = 2: queries
                     from 125 bp on take the 16-bit branch)
  kswa_oins0(_a2)    o_ins = 0, where the reference's lazy-F loop ends at its
                     first step and carries F into one column per block only
  kswa_asym, _odel0  del 5+3 / ins 8+1, and del 0+2 / ins 8+1
  kswa_xstop         KSW_XSTOP | v in the caller's xtra (the forward pass stops)
  kswa_long          queries of 200..256 bp, 16-bit
  kswa_edge_b, _w    query lengths around 8, 16 and 64 k against target lengths
                     0, 1 and around 64 k, byte and 16-bit; the 128-entry
                     suboptimal list
  kswa_sat(_a1)      byte scores at and just under the ceiling of 255
Bar: all seven kswr_t fields bit-exact, for the restatement (CPU) and the GPU's
wave routine (the one the alignment kernel runs, through smem_ksw_align2)."""
import gzip
import os

import numpy as np
import pytest

from oracle import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
BASE = ["kswa_a1", "kswa_a2"]
MORE = ["kswa_oins0", "kswa_oins0_a2", "kswa_asym", "kswa_odel0", "kswa_xstop", "kswa_long", "kswa_edge_b",
        "kswa_edge_w", "kswa_sat", "kswa_sat_a1"]
SETS = BASE + MORE
XBYTE, XSTOP, XSUBO, XSTART = 0x10000, 0x20000, 0x40000, 0x80000
GAPS = {"kswa_oins0": (6, 1, 0, 1), "kswa_oins0_a2": (12, 2, 0, 2), "kswa_asym": (5, 3, 8, 1),
        "kswa_odel0": (0, 2, 8, 1)}


def _load(name):
    from smemgpu import synth
    with gzip.open(os.path.join(HERE, "golden", name + ".smat.gz"), "rb") as fh:
        kb = synth.read_smat(fh.read())
    with gzip.open(os.path.join(HERE, "golden", name + ".smar.gz"), "rb") as fh:
        want = synth.read_smar(fh.read())
    return kb, want


def _same(got, want, kb=None):
    bad = np.nonzero(got != want)[0]
    if bad.size and kb is not None:
        for k in bad[:5]:
            print(f"task {k}: {kb.tasks[k]}\n  got  {got[k]}\n  want {want[k]}")
    for f in want.dtype.names:
        fb = np.nonzero(got[f] != want[f])[0]
        assert fb.size == 0, f"{f}: {fb.size} differ ({bad.size} results in all), first {fb[:5]}"


@pytest.mark.parametrize("name", SETS)
def test_kswa_fixture_shape(name):
    """Each set still holds the cases it was made for."""
    import dataclasses
    kb, want = _load(name)
    if name in BASE:
        assert kb.tasks.size == want.size == 3000
        byte = (kb.tasks["xtra"] & 0x10000) != 0
        if name == "kswa_a2":
            assert (~byte).sum() > 500          # the 16-bit branch runs
        assert (want["tb"] >= 0).sum() > 1000   # the start pass runs
        assert (want["score2"] > 0).sum() > 100  # suboptimal hits
        assert (want["te2"] >= 0).sum() > 100
        return
    assert 0 < kb.tasks.size == want.size <= 600
    byte = (kb.tasks["xtra"] & XBYTE) != 0
    qlen = kb.tasks["qlen"]
    if name in GAPS:
        assert (kb.o_del, kb.e_del, kb.o_ins, kb.e_ins) == GAPS[name]
        assert (want["tb"] >= 0).sum() > 200
    if name.startswith("kswa_oins0"):
        # problems where the reference's truncated lazy F and F carried across every block disagree
        full = oracle.ksw_align2(kb, full_f=True)
        assert (full != want).sum() >= 5
        assert (want["score2"] > 0).sum() > 100
    if name == "kswa_oins0_a2":
        assert (~byte).sum() > 100 and byte.sum() > 100
    if name == "kswa_xstop":
        assert ((kb.tasks["xtra"] & XSTOP) != 0).all()
        for flag in (XBYTE, XSUBO, XSTART):
            on = (kb.tasks["xtra"] & flag) != 0
            for v in (20, 40, 100):
                assert (on & ((kb.tasks["xtra"] & 0xffff) == v)).sum() >= 50
                assert (~on & ((kb.tasks["xtra"] & 0xffff) == v)).sum() >= 50
        free = dataclasses.replace(kb, tasks=kb.tasks.copy())
        free.tasks["xtra"] &= ~XSTOP
        assert (want["te"] < oracle.ksw_align2(free)["te"]).sum() >= 50
    if name == "kswa_long":
        assert (~byte).all() and qlen.min() >= 200 and qlen.max() == 256
        assert ((qlen >= 200) & (want["tb"] >= 0)).sum() >= 200
        assert (want["qe"] >= 192).sum() >= 200   # alignments that end in the fourth 64-column chunk
    if name.startswith("kswa_edge"):
        assert byte.all() if name == "kswa_edge_b" else (~byte).all()
        n = 18 * 7 * 3
        assert sorted(set(qlen[:n])) == [1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256]
        assert sorted(set(kb.tasks["tlen"][:n])) == [0, 1, 63, 64, 65, 255, 256]
        for ql in set(qlen[:n]):
            for tl in set(kb.tasks["tlen"][:n]):
                assert ((qlen[:n] == ql) & (kb.tasks["tlen"][:n] == tl)).sum() == 3
        assert (kb.q == 4).sum() >= 18 * 7   # the all-N queries
    if name == "kswa_edge_b":
        # `A` and `AC` against (AC)^128 with a threshold of 1: 128 list entries, the second
        # slot of the wave's per-lane list; score2 / te2 are the first entry outside the
        # best hit's window
        a, ac = kb.tasks[-2], kb.tasks[-1]
        assert (a["qlen"], a["tlen"], ac["qlen"], ac["tlen"]) == (1, 256, 2, 256)
        assert a["xtra"] == ac["xtra"] == XSUBO | XSTART | XBYTE | 1
        assert (want[-2]["score"], want[-2]["score2"], want[-2]["te2"]) == (1, 1, 2)
        assert (want[-1]["score"], want[-1]["score2"]) == (2, 2)
    if name.startswith("kswa_sat"):
        assert byte.all()
        assert (want["score"] == 255).sum() >= 20
        assert ((want["score"] >= 240) & (want["score"] <= 254)).sum() >= 20
        assert (want["qe"][want["score"] == 255] == -1).all()


@pytest.mark.parametrize("name", SETS)
def test_kswa_oracle_vs_reference(name):
    kb, want = _load(name)
    _same(oracle.ksw_align2(kb), want, kb)


def test_kswa_full_f_only_differs_at_oins0():
    """The test-only full-F variant of the restatement is the restatement
    itself wherever o_ins > 0 (the lazy-F loop's early exit loses nothing
    there), so what it shows on the o_ins = 0 sets is that exit alone."""
    for name in ("kswa_asym", "kswa_odel0", "kswa_long", "kswa_edge_b"):
        kb, want = _load(name)
        assert np.array_equal(oracle.ksw_align2(kb, full_f=True), want)


@pytest.fixture(scope="module")
def gpu(gpu_device):
    import smemgpu
    idx = smemgpu.Index.build(np.random.default_rng(1).integers(0, 4, 5000).astype(np.uint8))
    h = smemgpu.Gpu(idx, device=gpu_device)
    yield h
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_kswa_gpu_vs_reference(gpu, name):
    kb, want = _load(name)
    got, ms = gpu.ksw_align2(kb)
    _same(got, want, kb)


SCORINGS = {"default": (1, 4, 6, 1, 6, 1), "a2": (2, 8, 12, 2, 12, 2), "asym": (1, 4, 5, 3, 8, 1),
            "oins0": (1, 4, 6, 1, 0, 1), "odel0": (1, 4, 0, 2, 8, 1), "both0": (1, 4, 0, 1, 0, 1)}


@pytest.fixture(scope="module")
def fresh_genome():
    from smemgpu import synth
    return synth.make_genome(200_000, seed=171, n_chrom=1).codes


def _fresh_tasks(G, seed, a, b):
    """2000 problems: 1400 of synth.make_kswa_tasks' mix (< 200 bp) and 600
    queries of 200..256 bp with substitutions, indels and longer insertions,
    16-bit as the product would run them, one in five forced to bytes."""
    from smemgpu import synth
    short = synth.make_kswa_tasks(G, 1400, seed=seed, a=a, b=b)
    rng = np.random.default_rng(seed + 1000)
    tasks = np.zeros(2000, dtype=synth.KSWA_TASK)
    tasks[:1400] = short.tasks
    qs, ts = [short.q], [short.t]
    qo, to = short.q.size, short.t.size
    for k in range(1400, 2000):
        ql = int(rng.integers(200, 257))
        pos = int(rng.integers(300, G.size - 600))
        q = synth._mutated_copy(G[pos:pos + ql], rng, float(rng.choice([0.0, 0.02, 0.05])),
                                float(rng.choice([0.0, 0.01, 0.04])))
        if rng.random() < 0.5:
            at = int(rng.integers(1, q.size))
            q = np.concatenate([q[:at], rng.integers(0, 4, size=int(rng.integers(2, 9))).astype(np.uint8), q[at:]])
        q = np.concatenate([q, G[pos + ql:pos + ql + 60]])[:ql]   # exactly 200..256 bp
        lo = pos - int(rng.integers(0, 30))
        t = G[lo:lo + int(rng.integers(180, 257))]
        xtra = XSUBO | XSTART | 19 * a | (XBYTE if rng.random() < 0.2 else 0)
        tasks[k] = (qo, to, q.size, t.size, xtra, 0)
        qs.append(q)
        ts.append(t)
        qo += q.size
        to += t.size
    return synth.KswBatch(tasks, np.concatenate(qs).astype(np.uint8), np.concatenate(ts).astype(np.uint8),
                          synth.bwa_scmat(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("scoring", list(SCORINGS))
def test_kswa_gpu_vs_oracle(gpu, fresh_genome, scoring):
    """Fresh problems per scoring against the restatement (pinned to the
    reference by the sets above for each of these gap shapes)."""
    a, b, o_del, e_del, o_ins, e_ins = SCORINGS[scoring]
    kb = _fresh_tasks(fresh_genome, 172 + list(SCORINGS).index(scoring), a, b)
    kb.o_del, kb.e_del, kb.o_ins, kb.e_ins = o_del, e_del, o_ins, e_ins
    assert (kb.tasks["qlen"] >= 200).sum() == 600 and kb.tasks["qlen"].max() == 256
    got, ms = gpu.ksw_align2(kb)
    _same(got, oracle.ksw_align2(kb), kb)
    assert ms > 0


@pytest.mark.gpu
def test_kswa_rejects(gpu):
    import smemgpu
    from smemgpu import synth

    def batch(qlen=10, tlen=10, q_off=0, t_off=0, qpool=256, tpool=256, code=0, **pen):
        kb = synth.KswBatch(np.array([(q_off, t_off, qlen, tlen, XSUBO | XSTART | XBYTE | 19, 0)],
                                     dtype=synth.KSWA_TASK),
                            np.full(qpool, code, np.uint8), np.zeros(tpool, np.uint8), synth.bwa_scmat())
        for k, v in pen.items():
            setattr(kb, k, v)
        return kb

    got, _ = gpu.ksw_align2(batch(256, 256))   # the largest problem the entry point takes
    assert got.size == 1 and got[0]["score"] == 255
    for bad in (batch(qlen=0), batch(qlen=257, qpool=300), batch(tlen=257, tpool=300),
                batch(qlen=10, q_off=250), batch(tlen=10, t_off=250), batch(code=5), batch(e_ins=0), batch(e_del=0)):
        with pytest.raises(smemgpu.SmemError):
            gpu.ksw_align2(bad)
    e = synth.KswBatch(np.zeros(0, dtype=synth.KSWA_TASK), np.zeros(0, np.uint8), np.zeros(0, np.uint8),
                       synth.bwa_scmat())
    got, _ = gpu.ksw_align2(e)
    assert got.size == 0
