"""Reads of 321 bp to 70 kbp, on the CPU: the restatement against the compiled
reference's streams (tests/golden/long/), and the conditions on the inputs of
tests/test_gpu_long_reads.py that make its comparisons mean something.

The GPU tests compare with the restatement on fresh inputs; that the
restatement is the reference at these lengths is what the first test pins:
oracle.seed, OracleSA.lookup over oracle.sa_queries and oracle.chain (both
filter modes) equal the fixture's four streams byte for byte.
"""
import numpy as np
import pytest

import long_reads as LR
from oracle import oracle
from tests import golden_data


@pytest.fixture(scope="module")
def fixture_world(built, tmp_path_factory):
    """the restatement's lists, positions and unfiltered / filtered chains of the r5 reads on g1"""
    from smemgpu import synth
    p = golden_data.files("g1", str(tmp_path_factory.mktemp("g1")))
    oi, osa = oracle.OracleIndex(p["bwt"]), oracle.OracleSA(p["sa"])
    reads, names = golden_data.long_reads()
    case = golden_data.long_case()
    stream, per, st = oracle.seed(oi, reads.codes, reads.offs, threads=2, **case["opt"])
    lists = synth.read_smgo(stream)
    k = case["opt"]["min_seed_len"]
    counts, pos = LR.sa_truth(oi, osa, lists, k, case["max_occ"])
    chains = [LR.chain_truth(oi, osa, lists, golden_data.l_pac("g1"), k, case["max_occ"], filter=f) for f in (0, 1)]
    yield dict(reads=reads, names=names, case=case, stream=stream, per=per, st=st, lists=lists, counts=counts,
               pos=pos, chains=chains)
    oi.close()
    osa.close()


@pytest.fixture(scope="module")
def synth_world(built):
    """the same of the synthetic set on the planted genome, plus its chains at max_chain_gap 20000"""
    from smemgpu import synth
    w = LR.world()
    stream, per, st = LR.seed_truth(w, "all", w["reads"])
    lists = synth.read_smgo(stream)
    counts, pos = LR.sa_truth(w["oi"], w["osa"], lists, 19, 10000)
    chains = {gap: LR.chain_truth(w["oi"], w["osa"], lists, w["l_pac"], filter=0, max_chain_gap=gap)
              for gap in (10000, 20000)}
    return dict(w, stream=stream, per=per, st=st, lists=lists, counts=counts, pos=pos, chains=chains)


def test_fixture_manifest(fixture_world):
    f = fixture_world
    m = golden_data.long_manifest()
    assert f["reads"].n == m["reads"]["n_reads"] == len(f["names"]) == 16
    assert [int(x) for x in f["reads"].lens] == m["reads"]["lens"]
    lens = sorted(int(x) for x in f["reads"].lens)
    assert lens[:15] == sorted(2 * LR.CLASS_LENGTHS + [LR.LONG_LEN])
    assert LR.CHIMERA_MAIN + 600 <= lens[15] <= LR.CHIMERA_MAIN + 900


def test_restatement_equals_fixture(fixture_world):
    """oracle.seed / OracleSA.lookup / oracle.chain == `ref_harness smem / sa / chain`, byte for byte"""
    from smemgpu import synth
    f = fixture_world
    assert f["stream"] == golden_data.long_smgo()
    assert f["st"]["n_intv"] == f["case"]["n_intv"] and f["st"]["n_calls"] == f["case"]["n_calls"]
    assert synth.write_smsa(f["pos"]) == golden_data.long_smsa()
    assert int(f["counts"].sum()) == f["case"]["n_occ"]
    for filt in (0, 1):
        assert f["chains"][filt] == golden_data.long_smch(filt), filt


def _intervals(lists, i):
    """(begins, ends) of every interval of read i"""
    a = [c for c in lists[i] if c.shape[0]]
    info = np.concatenate([c[:, 3] for c in a]) if a else np.zeros(0, np.uint64)
    return (info >> np.uint64(32)).astype(np.int64), (info & np.uint64(0xFFFFFFFF)).astype(np.int64)


def test_inputs_reach_the_paths(fixture_world, synth_world):
    """Conditions on the inputs, from the fixture and the restatement alone (no GPU work): each names
    the code that only an input of this kind enters.  One that fails asks for other inputs."""
    from smemgpu import synth
    from test_gpu_seed_phases import ORC_NL, OWN_LIST
    f, s = fixture_world, synth_world
    sets = [(f["reads"], f["lists"], f["per"]), (s["reads"], s["lists"], s["per"])]
    # a query end past 2^16: the 16-base window arithmetic and `len - end` far inside one read
    assert any(_intervals(lists, i)[1].max(initial=0) >= 65536 for reads, lists, _ in sets for i in range(reads.n))
    # the 13-bit fields of the packed entry: bit 12 of a begin, and the largest end they hold
    short = [(lists, i) for reads, lists, _ in sets for i in range(reads.n) if reads.lens[i] <= 8191]
    assert any(_intervals(lists, i)[0].max(initial=0) >= 4096 for lists, i in short)
    assert any((_intervals(lists, i)[1] == 8191).any() for lists, i in short)
    # more than 2048 intervals in one read: intv_cap = 2 grows 8, 32, 128, 512, 2048, 8192 -- 6 overflow rounds
    assert max(int(per["n_intv"].max()) for _, _, per in sets) > 2048
    # more than 512 calls in one read: the raw log's call ordinal
    assert max(int(per["n_calls"].max()) for _, _, per in sets) > 512
    # no read fills the default capacity of a batch made for it
    for reads, _, per in sets:
        assert (per["n_intv"] <= reads.lens // 2 + 32).all()
    # a chain of 200 seeds or more: the linked-list walk of chain_weight
    all_chains = [synth.read_smch(f["chains"][0]), synth.read_smch(s["chains"][10000])]
    assert max(sd.size for per_read in all_chains for chains in per_read for _, sd in chains) >= 200
    # the chimeras: chains beside the long one, whose weight does not fit the wave sort's 16-bit key
    for names, per_read in ((f["names"], all_chains[0]), (s["names"], all_chains[1])):
        chains = per_read[names.index("chimera")]
        assert len(chains) >= 3
        assert max(LR.chain_weight(sd) for _, sd in chains) >= 65536
    # the gap read: max_chain_gap decides between two chains and one
    gi = s["names"].index("gap")
    n10, n20 = (len(synth.read_smch(s["chains"][gap])[gi]) for gap in (10000, 20000))
    assert n10 != n20 and n10 == 2 and n20 == 1
    # the reads across the tandem runs: forward lists past the LDS ring, and (the argument of
    # test_gpu_seed_phases.test_inputs_reach_the_paths) a backward step of more entries than an
    # owner's LDS list holds
    for name in ("hp", "di"):
        one = s["reads"].subset([s["names"].index(name)])
        _, st = oracle.seed_stats(s["oi"], one.codes, one.offs)
        assert st["n_fwd_spill"] > 0, name
        assert st["n_bwd_step"] > 0 and st["n_bwd_task_hi"] > st["n_bwd_step"] * (OWN_LIST - ORC_NL), (name, st)
    # the shapes the set promises
    lens = [int(x) for x in s["reads"].lens]
    assert {0, 1, 150, 2000, 5000, 27000, 70000} | set(LR.CLASS_LENGTHS) <= set(lens)
    assert lens.count(70000) == 3 and lens.count(150) == 100
