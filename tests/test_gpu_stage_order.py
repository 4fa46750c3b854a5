"""A batch's stage cursor (csrc/smem_gpu.cpp: stage_begin / stage_done): a stage needs its
predecessor's results on the batch, new reads or a re-run stage end everything after them, and
a stage that fails leaves the earlier stages' results fetchable.

Bar: exact.  Whatever a batch hands back after a refusal, a rewind or a failure equals, byte
for byte, what a fresh batch computes from the same reads.  One exception in form, none in
content: smem_batch_reg2aln places a record's CIGAR and MD in its pools by atomic cursors
(csrc/global_kernels.hip), so the pools' order is the scheduler's; an alignment is compared as
its fields without the two pool offsets, plus its own CIGAR words and MD bytes.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_READS, READ_LEN = 8, 100


class _Env:
    pass


@pytest.fixture(scope="module")
def env(gpu_device):
    """one handle (index, SA, .pac, one contig and its name), two read sets and the outputs a
    fresh batch computes for each"""
    import smemgpu
    from smemgpu import synth
    E = _Env()
    g = synth.make_genome(20_000, seed=31)
    idx, sa = smemgpu.Index.build_sa(g.codes)
    c = np.concatenate([g.codes, np.zeros((-g.codes.size) % 4, np.uint8)]).reshape(-1, 4).astype(np.uint8)
    pac = (c[:, 0] << 6 | c[:, 1] << 4 | c[:, 2] << 2 | c[:, 3]).astype(np.uint8)
    E.l_pac = int(g.codes.size)
    E.reads = [synth.make_reads(g.codes, N_READS, READ_LEN, seed=s) for s in (32, 33)]
    assert E.reads[0].codes.tobytes() != E.reads[1].codes.tobytes()
    E.names = [["a%d" % r for r in range(N_READS)], ["b%d" % r for r in range(N_READS)]]
    E.opt = smemgpu.aln_opt()
    E.gpu = smemgpu.Gpu(idx, device=gpu_device)
    try:
        E.gpu.load_sa(sa)
        E.gpu.load_pac(pac, E.l_pac)
        E.gpu.load_contigs([0], [E.l_pac], E.l_pac)
        E.gpu.load_contig_names(["chr1"])
        E.want = []
        for k in range(2):
            b = _batch(E)
            _forward(E, b, k, "reads")
            E.want.append(_outputs(b))
            b.close()
        assert all(len(w["regs"]) > 0 and len(w["sam"][0]) > 0 for w in E.want)
        yield E
    finally:
        E.gpu.close()


def _batch(E):
    return E.gpu.batch(N_READS, N_READS * READ_LEN, READ_LEN)


def _stages(E, b, k):
    """the stages in order, as (name, call); read set k"""
    return [("reads", lambda: (b.set_reads(E.reads[k].codes, E.reads[k].offs), b.set_read_text(E.names[k]))),
            ("run", lambda: b.run()),
            ("sa", lambda: b.sa(19, 10000)),
            ("chain", lambda: b.chain(E.l_pac)),
            ("chain2aln", lambda: b.chain2aln(E.opt)),
            ("reg_finalize", lambda: b.reg_finalize()),
            ("reg2aln", lambda: b.reg2aln(E.opt)),
            ("sam", lambda: b.sam())]


def _forward(E, b, k, first):
    """every stage from `first` on, in order"""
    names = [n for n, _ in _stages(E, b, k)]
    for _, call in _stages(E, b, k)[names.index(first):]:
        call()


def _fin_bytes(fin):
    return tuple(x.tobytes() for x in (fin.regs, fin.out_off, fin.sel, fin.sel_idx, fin.sel_off, fin.status))


def _aln_records(aln):
    """every record as (its fields without the pool offsets, its CIGAR words, its MD bytes)"""
    out = []
    for a in aln.alns:
        co, mo = int(a["cigar_off"]), int(a["md_off"])
        fields = tuple(int(a[f]) for f in ("pos", "is_rev", "n_cigar", "NM", "score", "tries", "status", "md_len"))
        out.append((fields, aln.cigar[co:co + int(a["n_cigar"])].tobytes(), aln.md[mo:mo + int(a["md_len"])].tobytes()))
    return out, aln.rid.tobytes(), aln.aln_off.tobytes(), aln.cigar.size, aln.md.size


def _seed_bytes(res):
    return tuple(x.tobytes() for x in (res.intv, res.intv_off, res.call_n, res.call_off, res.occ_off, res.sa_pos,
                                       res.chain_off, res.chains, res.seeds))


def _outputs(b):
    """the regions, final regions, alignments and SAM text of a batch that has run through sam"""
    from smemgpu.lib import FETCH_ALN, FETCH_FIN, FETCH_REGS, FETCH_SAM
    res = b.fetch(FETCH_REGS | FETCH_FIN | FETCH_ALN | FETCH_SAM)
    return {"regs": res.regs.tobytes(), "reg_off": res.reg_off.tobytes(), "fin": _fin_bytes(res.fin),
            "aln": _aln_records(res.aln),
            "sam": (res.sam.text.tobytes(), res.sam.text_off.tobytes(), res.sam.status.tobytes())}


def _refused(call):
    import smemgpu
    with pytest.raises(smemgpu.SmemError, match="SMEM_E_ARG"):
        call()


def test_new_reads_end_every_stage(env):
    """after set_reads on a used batch every stage and every fetch is refused until the batch
    has run again (chain, reg_finalize and reg2aln used to pass their guards and compute over
    the previous reads' intervals and regions); the chain run in order then equals a fresh batch's"""
    from smemgpu.lib import (FETCH_ALL, FETCH_ALN, FETCH_CHAINS, FETCH_FIN, FETCH_INTV, FETCH_REGS, FETCH_SA,
                             FETCH_SAM)
    E = env
    b = _batch(E)
    try:
        _forward(E, b, 0, "reads")
        b.fetch()
        assert _outputs(b) == E.want[0]
        b.set_reads(E.reads[1].codes, E.reads[1].offs)
        for name, call in _stages(E, b, 1)[2:]:
            _refused(call)
        for mask in (None, FETCH_INTV, FETCH_SA, FETCH_CHAINS, FETCH_REGS, FETCH_ALL, FETCH_FIN, FETCH_ALN, FETCH_SAM,
                     FETCH_ALL | FETCH_FIN | FETCH_ALN | FETCH_SAM):
            _refused(lambda: b.fetch(mask))
        assert E.gpu.fault()[0] == 0
        b.set_read_text(E.names[1])
        _forward(E, b, 1, "run")
        assert _outputs(b) == E.want[1]
    finally:
        b.close()


def test_stage_order(env):
    """on a fresh batch every stage is refused before its predecessor has run and accepted after"""
    E = env
    b = _batch(E)
    try:
        stages = _stages(E, b, 0)
        for i, (name, call) in enumerate(stages):
            # stages[i]'s predecessor has run, stages[i] has not: everything after it is refused
            # (smem_batch_run itself asks for nothing: a batch without reads seeds none)
            for _, later in stages[max(i + 1, 2):]:
                _refused(later)
            call()
        assert E.gpu.fault()[0] == 0
        assert _outputs(b) == E.want[0]
    finally:
        b.close()


def test_rerun_stage_ends_later_stages(env):
    """chain run again: the regions, final regions, alignments and text are refused, the
    intervals, positions and chains come back as before; run forward again, all equal the first"""
    from smemgpu.lib import FETCH_ALN, FETCH_CHAINS, FETCH_FIN, FETCH_INTV, FETCH_REGS, FETCH_SA, FETCH_SAM
    E = env
    b = _batch(E)
    try:
        _forward(E, b, 0, "reads")
        seeds0 = _seed_bytes(b.fetch(FETCH_INTV | FETCH_SA | FETCH_CHAINS))
        assert _outputs(b) == E.want[0]
        b.chain(E.l_pac)
        for mask in (FETCH_REGS, FETCH_FIN, FETCH_ALN, FETCH_SAM):
            _refused(lambda: b.fetch(mask))
        assert _seed_bytes(b.fetch(FETCH_INTV | FETCH_SA | FETCH_CHAINS)) == seeds0
        _forward(E, b, 0, "chain2aln")
        assert _outputs(b) == E.want[0]
        assert _seed_bytes(b.fetch(FETCH_INTV | FETCH_SA | FETCH_CHAINS)) == seeds0
    finally:
        b.close()


def test_results_survive_a_later_stage_failing(env):
    """SMEM_GPU_FAIL=g2a:1 (a return code after the work is enqueued, not a device fault):
    reg2aln fails, the final regions stay fetchable and unchanged, the alignments are refused,
    and without the variable the stage runs"""
    import smemgpu
    from smemgpu.lib import FETCH_ALN, FETCH_FIN
    E = env
    b = _batch(E)
    old = os.environ.get("SMEM_GPU_FAIL")
    try:
        for _, call in _stages(E, b, 0)[:6]:
            call()
        fin0 = _fin_bytes(b.fetch(FETCH_FIN).fin)
        assert fin0 == E.want[0]["fin"]
        os.environ["SMEM_GPU_FAIL"] = "g2a:1"
        with pytest.raises(smemgpu.SmemError, match="SMEM_E_DEVICE.*injected"):
            b.reg2aln(E.opt)
        assert _fin_bytes(b.fetch(FETCH_FIN).fin) == fin0
        _refused(lambda: b.fetch(FETCH_ALN))
        _refused(lambda: b.sam())
        os.environ.pop("SMEM_GPU_FAIL")
        assert E.gpu.fault()[0] == 0
        _forward(E, b, 0, "reg2aln")
        assert _outputs(b) == E.want[0]
    finally:
        if old is None:
            os.environ.pop("SMEM_GPU_FAIL", None)
        else:
            os.environ["SMEM_GPU_FAIL"] = old
        b.close()
