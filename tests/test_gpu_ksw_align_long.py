"""smem_ksw_align2_long on the GPU: ksw_align2 with targets of up to
SMEM_KSWA_MAX_TLEN bases (kswd::sw_pass_wave<true>: the target fetched 64 rows
at a time, the suboptimal list in LDS).  Bar: every kswr_t field equal to the
reference's (the kswa_msw sets) and to the restatement that those sets pin
(fresh problems per scoring of test_ksw_align.SCORINGS)."""
import numpy as np
import pytest

from oracle import oracle
from tests import msw_data
from tests.test_ksw_align import SCORINGS, XBYTE, XSTART, XSUBO

pytestmark = pytest.mark.gpu
MAX = msw_data.MAX_TLEN


@pytest.fixture(scope="module")
def gpu(gpu_device):
    import smemgpu
    idx = smemgpu.Index.build(np.random.default_rng(1).integers(0, 4, 5000).astype(np.uint8))
    h = smemgpu.Gpu(idx, device=gpu_device)
    yield h
    h.close()


@pytest.fixture(scope="module")
def fresh_genome():
    from smemgpu import synth
    return synth.make_genome(200_000, seed=191, n_chrom=1).codes


@pytest.mark.parametrize("name", msw_data.KSWA_SETS)
def test_kswa_long_gpu_vs_reference(gpu, name):
    kb, want = msw_data.load_kswa(name)
    got, ms = gpu.ksw_align2_long(kb)
    msw_data.same(got, want, kb)
    assert ms > 0


def _fresh_tasks(G, seed, a, b):
    """1000 problems with targets of 257..MAX bases: 700 rescue-shaped (a read
    of 30..256 bp with substitutions and indels, one in four with a longer
    insertion, against a window that holds it or cuts it, half of them
    reverse-complemented), 200 of random lengths with a second, weaker copy of
    the read elsewhere in the window, 100 at the length limits; byte or 16-bit
    by mem_matesw's rule, one in five forced to bytes."""
    from smemgpu import synth
    rng = np.random.default_rng(seed)
    tasks = np.zeros(1000, dtype=synth.KSWA_TASK)
    qs, ts = [], []
    qo = to = 0
    for k in range(1000):
        if k < 900:
            ql = int(rng.integers(30, 257))
            wl = int(rng.integers(257, MAX + 1)) if k % 3 else int(rng.integers(400, 1501))
        else:
            ql = int(rng.choice([1, 2, 63, 64, 65, 255, 256]))
            wl = int(rng.choice([257, 320, MAX - 64, MAX - 1, MAX]))
        pos = int(rng.integers(0, G.size - wl))
        t = G[pos:pos + wl].copy()
        at = int(rng.integers(-20, wl - ql // 2))
        src = t[max(at, 0):at + ql + 30]
        q = synth._mutated_copy(src, rng, float(rng.choice([0.0, 0.02, 0.05, 0.1])), float(rng.choice([0.0, 0.01, 0.04])))
        if k % 4 == 0 and q.size > 2:
            cut = int(rng.integers(1, q.size))
            q = np.concatenate([q[:cut], rng.integers(0, 4, size=int(rng.integers(2, 9))).astype(np.uint8), q[cut:]])
        q = np.concatenate([q, rng.integers(0, 4, size=ql).astype(np.uint8)])[:ql]
        if 700 <= k < 900:   # a second, weaker copy
            w = synth._mutated_copy(q, rng, 0.08, 0.01)[:max(1, wl - 1)]
            p2 = int(rng.integers(0, wl - w.size + 1))
            t[p2:p2 + w.size] = w
        if rng.random() < 0.02:
            q[rng.random(q.size) < 0.05] = 4
        if k % 2:
            q, t = (3 - np.minimum(q, 3))[::-1].astype(np.uint8), (3 - t)[::-1].astype(np.uint8)
        byte = ql * a < 250 or rng.random() < 0.2
        minsc = 19 * a if k % 10 else int(rng.integers(1, 8))
        tasks[k] = (qo, to, q.size, t.size, XSUBO | XSTART | (XBYTE if byte else 0) | minsc, 0)
        qs.append(q)
        ts.append(t)
        qo += q.size
        to += t.size
    return synth.KswBatch(tasks, np.concatenate(qs).astype(np.uint8), np.concatenate(ts).astype(np.uint8),
                          synth.bwa_scmat(a, b))


@pytest.mark.parametrize("scoring", list(SCORINGS))
def test_kswa_long_gpu_vs_oracle(gpu, fresh_genome, scoring):
    a, b, o_del, e_del, o_ins, e_ins = SCORINGS[scoring]
    kb = _fresh_tasks(fresh_genome, 192 + list(SCORINGS).index(scoring), a, b)
    kb.o_del, kb.e_del, kb.o_ins, kb.e_ins = o_del, e_del, o_ins, e_ins
    T = kb.tasks
    assert T.size == 1000 and T["tlen"].min() >= 257 and T["tlen"].max() == MAX and T["qlen"].max() == 256
    want = oracle.ksw_align2(kb)
    assert (want["tb"] >= 0).sum() >= 400 and (want["te2"] >= 0).sum() >= 100
    got, ms = gpu.ksw_align2_long(kb)
    msw_data.same(got, want, kb)


def test_kswa_long_takes_short_targets(gpu):
    """tlen <= 256 is accepted and gives what the short entry point gives"""
    from tests.test_ksw_align import _load
    kb, want = _load("kswa_edge_b")
    assert kb.tasks["tlen"].max() == 256 and kb.tasks["tlen"].min() == 0
    got, _ = gpu.ksw_align2_long(kb)
    short, _ = gpu.ksw_align2(kb)
    msw_data.same(got, short, kb)
    msw_data.same(got, want, kb)


def test_kswa_long_rejects(gpu):
    import smemgpu
    from smemgpu import synth

    def batch(qlen=10, tlen=300, q_off=0, t_off=0, qpool=256, tpool=MAX, code=0, **pen):
        kb = synth.KswBatch(np.array([(q_off, t_off, qlen, tlen, XSUBO | XSTART | XBYTE | 19, 0)],
                                     dtype=synth.KSWA_TASK),
                            np.full(qpool, code, np.uint8), np.zeros(tpool, np.uint8), synth.bwa_scmat())
        for k, v in pen.items():
            setattr(kb, k, v)
        return kb

    got, _ = gpu.ksw_align2_long(batch(256, MAX))   # the largest problem the entry point takes
    assert got.size == 1 and got[0]["score"] == 255
    for bad in (batch(tlen=MAX + 1, tpool=MAX + 64), batch(qlen=257, qpool=300), batch(qlen=0), batch(code=5),
                batch(e_ins=0), batch(e_del=0), batch(qlen=10, q_off=250), batch(tlen=300, t_off=MAX - 100)):
        with pytest.raises(smemgpu.SmemError):
            gpu.ksw_align2_long(bad)
    e = synth.KswBatch(np.zeros(0, dtype=synth.KSWA_TASK), np.zeros(0, np.uint8), np.zeros(0, np.uint8),
                       synth.bwa_scmat())
    got, _ = gpu.ksw_align2_long(e)
    assert got.size == 0
