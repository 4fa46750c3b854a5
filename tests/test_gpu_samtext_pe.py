"""Paired-end SAM text on the GPU (smem_sam_text_pe over host buffers; the paired-end kernels of
csrc/sam_kernels.hip).

Bar: exact.  (a) The three fixture sets (tests/golden/sampe/sampe, tests/golden/pair/rep and
rep_a2) go from the reference's raw regions to its SAM through library calls alone -- pestat,
matesw, reg_finalize, pair, reg2aln, sam_text_pe; tests/sampe_chain.py does the host-side
assembly between them -- and every line of every pair the chain keeps equals the reference's,
byte for byte.  (b)-(e) Synthetic records at the smallest shapes at which the kernels can go
wrong equal the restatement (tests/samtext_pe_ref.py, pinned to the reference in
tests/test_samtext_pe.py).  p0 == p1, RG:Z, comments, 0x100 and 0x10000 records rest on the
restatement's reading alone.
"""
import numpy as np
import pytest

import test_gpu_samtext as G
from tests import samtext_pe_ref as R

pytestmark = pytest.mark.gpu

CTG_NAMES, CTG_OFFS = G.CTG_NAMES, G.CTG_OFFS
FAR = 3                                             # the contig whose offset is beyond 2^32


@pytest.fixture(scope="module")
def gpu(gpu_device):
    import smemgpu
    from smemgpu import synth
    h = smemgpu.Gpu(smemgpu.Index.build(synth.make_genome(2000, seed=3).codes), device=gpu_device)
    yield h
    h.close()


# ------------------------------------------------------------------ (a) the fixture sets, through library calls alone
@pytest.mark.parametrize("name", ["sampe", "rep", "rep_a2"])
def test_library_chain_gives_the_reference_sam(gpu, name):
    from smemgpu.lib import SAM_HOST
    from tests import pair_chain as PC, sampe_chain as SC
    F = SC.load(name)
    got, sel = SC.library(gpu, F)
    n_pairs = F["man"]["pairs"]
    assert got.text_off.size == 2 * n_pairs + 1 and sel.size == n_pairs
    host = [p for p in range(n_pairs) if got.status[2 * p] == SAM_HOST]
    assert host == SC.HOST_PAIRS[name] and len(host) <= PC.MAX_HOST_FRACTION * n_pairs
    branches = {int(b) for b in sel["branch"]}
    print(f"sam_text_pe {name}: {got.text.size} B, {len(host)} pairs to the host, branches {sorted(branches)}, "
          f"kernels {got.kernel_ms:.3f} ms")
    assert branches >= {0, 1} and (name == "sampe" or 2 in branches)
    for r, w in enumerate(F["want"]):
        if r >> 1 in host:
            assert got.status[r] == SAM_HOST and got.read(r) == b""
            continue
        assert got.status[r] == 0 and got.read(r) == w, (name, r, got.read(r), w)
    # the text can be written to a file as it is: the reference's SAM without its header
    if not host:
        assert got.text.tobytes() == b"".join(F["want"])
    assert gpu.fault()[0] == 0


# ------------------------------------------------------------------ synthetic pairs
def _sel(branch=0, proper=0, mapq=(-1, -1), status=0):
    return dict(status=status, branch=branch, proper=proper, mapq=list(mapq))


def _add(pairs, rng, L0, L1, recs0, recs1, sel, name=None, **kw):
    """a pair: two reads of one name (1 to 40 bytes by the pair's number), comments of their own"""
    i = len(pairs)
    name = name if name is not None else "p" * (i % 40 + 1)
    a = G._read(rng, 2 * i, L0, recs0, name=name, fin_status=kw.get("fin0", 0))
    b = G._read(rng, 2 * i + 1, L1, recs1, name=name, fin_status=kw.get("fin1", 0))
    pairs.append(((a, b), sel))


def _combo_pairs():
    """every combination of mapped / unmapped ends, strand, same or other contig, branch and proper,
    with 1 to 4 records a read in branch 0 and reads of 1 to 300 bp"""
    rng = np.random.default_rng(31)
    pairs = []
    lens = (1, 2, 7, 8, 15, 16, 17, 33, 63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 299, 300)
    for branch in (0, 1, 2):
        states = ("u", "f", "r") if branch == 0 else ("f", "r")
        for s0 in states:
            for s1 in states:
                for other in (0, 1):
                    for proper in (0, 1):
                        i = len(pairs)
                        L = [lens[i % len(lens)], lens[(3 * i + 5) % len(lens)]]
                        rid = [int(rng.integers(0, 5))] * 2
                        if other:
                            rid[1] = (rid[0] + 1 + int(rng.integers(0, 4))) % 5
                        recs = []
                        for e, s in enumerate((s0, s1)):
                            if s == "u":
                                recs.append([])
                                continue
                            n = 1 if branch or L[e] < 8 else 1 + (i + e) % 4
                            lst = [G._rec(rng, L[e], k, rid=rid[e] if k == 0 else int(rng.integers(0, 5)),
                                          is_rev=int(s == "r") if k == 0 else int(rng.integers(0, 2))) for k in range(n)]
                            recs.append(lst)
                        mapq = (int(rng.integers(0, 61)), int(rng.integers(0, 61))) if branch else (-1, -1)
                        _add(pairs, rng, L[0], L[1], recs[0], recs[1], _sel(branch, proper, mapq))
    return pairs


def _edge_pairs():
    rng = np.random.default_rng(32)
    pairs = []
    M = lambda L, **kw: G._rec(rng, L, 0, n_words=1, clip5=0, clip3=0, **kw)   # noqa: E731  (one M word: rlen == L)
    # PNEXT at each digit boundary (10^k - 1 and 10^k, k = 1..10), on the contig beyond 2^32 and on another
    for k in range(1, 11):
        for v in (10 ** k - 1, 10 ** k):
            _add(pairs, rng, 50, 50, [M(50, rid=FAR, pos1=5, is_rev=0)], [M(50, rid=FAR, pos1=v, is_rev=1)], _sel(0, 1))
            _add(pairs, rng, 50, 50, [M(50, rid=1, pos1=77, is_rev=1)], [M(50, rid=FAR, pos1=v, is_rev=0)], _sel(2, 0, (9, 10)))
    # |TLEN| at each digit boundary, both signs: forward ends t - 1 apart; reverse ends likewise
    for k in range(1, 11):
        for t in (10 ** k - 1, 10 ** k):
            _add(pairs, rng, 30, 30, [M(30, rid=FAR, pos1=3, is_rev=0)], [M(30, rid=FAR, pos1=3 + t - 1, is_rev=0)], _sel(1, 1, (60, 0)))
            _add(pairs, rng, 30, 40, [M(30, rid=4, pos1=3 + t - 1, is_rev=1)], [M(40, rid=4, pos1=3 + 10, is_rev=1)], _sel(0, 0))
    # TLEN 0: equal 5' ends -- two forward reads at one place; two reverse reads that end at one place
    _add(pairs, rng, 30, 60, [M(30, rid=2, pos1=500, is_rev=0)], [M(60, rid=2, pos1=500, is_rev=0)], _sel(0, 1))
    _add(pairs, rng, 30, 60, [M(30, rid=2, pos1=530, is_rev=1)], [M(60, rid=2, pos1=500, is_rev=1)], _sel(1, 1, (1, 2)))
    _add(pairs, rng, 30, 30, [M(30, rid=2, pos1=529, is_rev=0)], [M(30, rid=2, pos1=500, is_rev=1)], _sel(2, 0, (3, 4)))
    # CIGARs with D and I (and clips) on reverse records, the mate forward and reverse
    for n_words, c5, c3 in ((5, 0, 0), (7, 4, 0), (9, 3, 6), (8, 0, 11)):
        for mrev in (0, 1):
            a = G._rec(rng, 120, 0, rid=1, pos1=400, is_rev=1, n_words=n_words, clip5=c5, clip3=c3)
            b = G._rec(rng, 90, 0, rid=1, pos1=200, is_rev=mrev, n_words=n_words - 2, clip5=0, clip3=c3)
            assert any((w & 0xf) in (1, 2) for w in a.cigar)
            _add(pairs, rng, 120, 90, [a], [b], _sel(1, 1, (20, 30)))
    # supplementary, 0x100 and 0x10000 records in a pair; a supplementary line on another contig than the mate
    _add(pairs, rng, 100, 100, [G._rec(rng, 100, 0, rid=0), G._rec(rng, 100, 1, rid=0), G._rec(rng, 100, 2, rid=2)],
         [G._rec(rng, 100, 0, rid=0)], _sel(0, 1))
    _add(pairs, rng, 100, 100, [G._rec(rng, 100, 0, rid=1)],
         [G._rec(rng, 100, 0, rid=1), G._rec(rng, 100, 1, flag=0x100, xs=-1, mapq=0), G._rec(rng, 100, 2, rid=1)], _sel(0, 1))
    _add(pairs, rng, 100, 100, [G._rec(rng, 100, 0, xs=-1), G._rec(rng, 100, 1, flag=0x10000), G._rec(rng, 100, 2, flag=0x10000, xs=-1)],
         [G._rec(rng, 100, 0), G._rec(rng, 100, 1, flag=0x100, xs=-1, mapq=0)], _sel(0, 0))
    _add(pairs, rng, 100, 100, [G._rec(rng, 100, 0), G._rec(rng, 100, 1), G._rec(rng, 100, 2), G._rec(rng, 100, 3)], [], _sel(0, 1))
    # proper = 1 where 0x2 must stay clear: different contigs; an unmapped end; both unmapped
    _add(pairs, rng, 80, 80, [M(80, rid=0)], [M(80, rid=1)], _sel(0, 1))
    _add(pairs, rng, 80, 80, [M(80, rid=0)], [], _sel(0, 1))
    _add(pairs, rng, 80, 80, [], [], _sel(0, 1))
    # a placed unmapped read of 1 bp and of 300 bp on a reverse mate (and on a forward one), either end
    for L in (1, 300):
        for rev in (1, 0):
            _add(pairs, rng, L, 100, [], [G._rec(rng, 100, 0, is_rev=rev)], _sel(0, 0))
            _add(pairs, rng, 100, L, [G._rec(rng, 100, 0, is_rev=rev, rid=FAR, pos1=10 ** 10)], [], _sel(0, 0))
    _add(pairs, rng, 33, 33, [M(33)], [M(33)], _sel(1, 1, (5, 6)), name="n" * 255)
    return pairs


HOST_CAUSES = ("status", "mapq", "fin", "empty", "sel", "sel_mapq")


def _host_pairs():
    """each cause of SMEM_SAM_HOST in one end only, between pairs that stay"""
    rng = np.random.default_rng(33)
    pairs = []
    good = lambda: _add(pairs, rng, 40, 41, [G._rec(rng, 40, 0)], [G._rec(rng, 41, 0), G._rec(rng, 41, 1)], _sel(0, 1))   # noqa: E731
    good()
    _add(pairs, rng, 50, 50, [G._rec(rng, 50, 0)], [G._rec(rng, 50, 0), R.Rec(status=4, rid=-1, pos=-1, mapq=3, flag=0x800, score=40, xs=0)],
         _sel(0, 0))
    good()
    _add(pairs, rng, 50, 50, [G._rec(rng, 50, 0, mapq=-1)], [G._rec(rng, 50, 0)], _sel(0, 0))
    good()
    _add(pairs, rng, 50, 50, [G._rec(rng, 50, 0)], [G._rec(rng, 50, 0)], _sel(0, 0), fin1=1)
    good()
    _add(pairs, rng, 0, 50, [], [G._rec(rng, 50, 0)], _sel(0, 0))
    good()
    _add(pairs, rng, 50, 50, [G._rec(rng, 50, 0)], [G._rec(rng, 50, 0)], _sel(0, 0, status=1))
    good()
    _add(pairs, rng, 50, 50, [G._rec(rng, 50, 0)], [G._rec(rng, 50, 0)], _sel(2, 0, (7, -1)))
    good()
    return pairs


def _many_pairs(n=5000):
    rng = np.random.default_rng(34)
    pairs = []
    for _ in range(n):
        L = [int(rng.integers(1, 90)), int(rng.integers(1, 90))]
        branch = int(rng.integers(0, 3))
        recs = []
        for e in range(2):
            k = 1 if branch else int(rng.integers(0, 4)) if L[e] >= 8 else int(rng.integers(0, 2))
            recs.append([G._rec(rng, L[e], j, flag=0x800 if j else 0) for j in range(k)])
        _add(pairs, rng, L[0], L[1], recs[0], recs[1],
             _sel(branch, int(rng.integers(0, 2)), (int(rng.integers(0, 61)), int(rng.integers(0, 61))) if branch else (-1, -1)))
    return pairs


def _pack(pairs):
    from smemgpu.lib import PAIR_SEL_DT
    reads = [r for rd, _s in pairs for r in rd]
    sel = np.zeros(len(pairs), dtype=PAIR_SEL_DT)
    for p, (_rd, s) in enumerate(pairs):
        sel[p]["status"], sel[p]["branch"], sel[p]["proper"], sel[p]["mapq"] = s["status"], s["branch"], s["proper"], s["mapq"]
    return reads, G._pack(reads), sel


def _want(pairs, qual=True, comments=True, rg_id=None):
    out = []
    for rd, s in pairs:
        t = R.pair_text(rd, s, CTG_NAMES, CTG_OFFS, rg_id, qual, comments)
        out += t if t is not None else [None, None]
    return out


def _call(gpu, A, sel, qual=True, comments=True, rg_id=None, **kw):
    return gpu.sam_text_pe(sel, A["codes"], A["offs"], A["names"], A["quals"] if qual else None,
                           A["comments"] if comments else None, A["aln_off"], A["alns"], A["rid"], A["recs"], A["cigar"],
                           A["md"], CTG_OFFS, CTG_NAMES, fin_status=A["fin_status"], rg_id=rg_id, **kw)


@pytest.fixture(scope="module")
def synthetic():
    pairs = _combo_pairs() + _edge_pairs()
    return pairs, _pack(pairs)


def test_synthetic_pairs_cover_the_cases(synthetic):
    """the fixture itself, read from the restatement's lines: every flag class, RNEXT at every
    offset mod 16, PNEXT and |TLEN| of 1 to 11 digits, TLEN 0 beside '=', both placed strands"""
    pairs, _ = synthetic
    want = _want(pairs)
    at, rnext_at, flags, pn, tl = 0, set(), set(), set(), set()
    zero_eq = named = 0
    for w in want:
        for line in w.split(b"\n")[:-1]:
            f = line.split(b"\t")
            rnext_at.add((at + sum(len(x) + 1 for x in f[:6])) % 16)
            fl = int(f[1])
            flags.add(fl & (0x1 | 0x2 | 0x4 | 0x8 | 0x10 | 0x20 | 0x40 | 0x80))
            if f[6] != b"*":
                pn.add(len(f[7]))
                tl.add(len(f[8].lstrip(b"-")) * (-1 if f[8].startswith(b"-") else 1))
                zero_eq += f[6] == b"=" and f[8] == b"0" and not fl & 0xc
                named += f[6] != b"="
            at += len(line) + 1
    assert rnext_at == set(range(16))
    assert pn >= set(range(1, 12)) and tl >= set(range(-11, 12)) - {0} and zero_eq >= 3 and named >= 20
    for need in (99, 147, 83, 163, 73, 133, 121, 185, 117, 181, 69, 137, 77, 141, 97, 145, 65, 129, 67, 131, 115, 179):
        assert need in flags, need
    assert {len(rd[e]["name"]) for rd, _ in pairs for e in range(2)} >= set(range(1, 41))
    assert {len(rd[e]["codes"]) for rd, _ in pairs for e in range(2)} >= {1, 300}
    assert {len(rd[e]["recs"]) for rd, _ in pairs for e in range(2)} == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("qual,comments,rg_id", [(True, True, "grp1"), (True, False, None), (False, True, None),
                                                 (False, False, "a-long-read-group.id")])
def test_synthetic_pairs(gpu, synthetic, qual, comments, rg_id):
    pairs, (_reads, A, sel) = synthetic
    got = _call(gpu, A, sel, qual, comments, rg_id)
    G._same(got, _want(pairs, qual, comments, rg_id))
    assert got.kernel_ms > 0 and gpu.fault()[0] == 0


def test_single_end_call_on_the_same_records(gpu, synthetic):
    """smem_sam_text over the very same buffers still prints the single-end lines"""
    pairs, (reads, A, _sel_) = synthetic
    G._same(G._call(gpu, A), G._want(reads))


def test_host_pairs_and_neighbours(gpu):
    """each cause of SMEM_SAM_HOST, in one end only: both ends get zero bytes, the pairs around keep theirs"""
    from smemgpu.lib import SAM_HOST
    pairs = _host_pairs()
    _reads, A, sel = _pack(pairs)
    got, want = _call(gpu, A, sel), _want(pairs)
    G._same(got, want)
    host = [p for p in range(len(pairs)) if want[2 * p] is None]
    assert len(host) == len(HOST_CAUSES) and host == list(range(1, len(pairs), 2))
    for p in host:
        for r in (2 * p, 2 * p + 1):
            assert got.status[r] == SAM_HOST and got.text_off[r] == got.text_off[r + 1]
        for q in (p - 1, p + 1):
            assert got.read(2 * q) == want[2 * q] and got.read(2 * q + 1) == want[2 * q + 1] and want[2 * q]


def test_argument_errors(gpu):
    """every SMEM_E_ARG case of the paired-end call, and one of smem_sam_text's own"""
    import smemgpu
    rng = np.random.default_rng(35)

    def base(branch=0):
        pairs = []
        for _ in range(3):
            _add(pairs, rng, 30, 30, [G._rec(rng, 30, 0)], [G._rec(rng, 30, 0)], _sel(branch, 0, (1, 2) if branch else (-1, -1)))
        return pairs

    def refused(pairs, sel=None, match="SMEM_E_ARG"):
        _r, A, s = _pack(pairs)
        with pytest.raises(smemgpu.SmemError, match=match):
            _call(gpu, A, s if sel is None else sel)

    good = base()
    _r, A, s = _pack(good)
    refused(base(), sel=s[:2])                                          # n_reads != 2 * n_pairs
    refused(base(), sel=np.concatenate([s, s[:1]]))
    p = base()
    p[1][0][1]["name"] = p[1][0][1]["name"][:-1] + "Q"                  # the two names differ, same length
    refused(p)
    p = base()
    p[2][0][0]["name"] += "x"                                           # ... and in length
    refused(p)
    for n0, n1 in ((0, 1), (1, 0), (2, 1), (1, 2)):                     # branch 1 and 2 print exactly one record a read
        for branch in (1, 2):
            p = base(branch)
            p[1][0][0]["recs"] = [G._rec(rng, 30, k) for k in range(n0)]
            p[1][0][1]["recs"] = [G._rec(rng, 30, k) for k in range(n1)]
            refused(p)
    for branch in (-1, 3):
        p = base()
        p[0][1]["branch"] = branch
        refused(p)
    p = base()
    p[0][0][0]["codes"][3] = 5                                          # smem_sam_text's own: a code above 4
    refused(p)
    assert gpu.fault()[0] == 0
    G._same(_call(gpu, A, s), _want(good))                              # and the handle still works


def test_many_pairs_and_capacity(gpu):
    """5000 pairs: the write kernel's grid takes reads in turn; SMEM_E_CAPACITY reports the size a
    retry needs and the retry succeeds; an empty batch"""
    import smemgpu
    pairs = _many_pairs()
    _reads, A, sel = _pack(pairs)
    assert 2 * len(pairs) > 4096                                        # SAM_WRITE_BLOCKS_MAX
    want = _want(pairs)
    total = sum(len(w) for w in want if w)
    with pytest.raises(smemgpu.SmemError, match="SMEM_E_CAPACITY") as e:
        _call(gpu, A, sel, text_cap=total - 1, grow=False)
    assert e.value.n_bytes == total
    G._same(_call(gpu, A, sel, text_cap=total, grow=False), want)
    G._same(_call(gpu, A, sel, text_cap=16), want)                      # the binding's own retry
    _r, none, nosel = _pack([])
    got = _call(gpu, none, nosel)
    assert got.text.size == 0 and got.text_off.tolist() == [0] and got.status.size == 0
    assert gpu.fault()[0] == 0
