"""Regions -> alignments (smem_reg2aln) where no read of the fixtures goes: the
band-doubling retries of the 16- and 32-lane kernels on rows of several passes,
a deferral from each lane-group class into the scratch-tier kernel, and a
scratch tier with more regions than blocks, so that its grid loops and a slab
is reused by matrices of different row widths.

Bar: exact, every smem_aln_t field against tests/reg2aln_ref.py.  The CPU test
holds every synthetic region to the path it is named after, judged by the
restated classifier (reg2aln_ref.classify) and the restatement's tries; the GPU
test runs no region without that assertion.

A retry shape is m1 matched / i inserted / m2 matched / d deleted / m3 matched
bases at a truesc that makes infer_bw ask for a first band too narrow for the
gaps.  Equal lengths cannot start in the 16-lane class and retry (infer_bw gives
0 or at least 8 there), so retry16 and defer16 differ by one base.
"""
import functools
import re

import numpy as np
import pytest

import reg2aln_ref as ref
import test_reg2aln as T

OPTS = {"default": ref.Opt(), "gaps": ref.Opt(o_del=5, e_del=3, o_ins=8, e_ins=2)}

# name -> scoring -> (shape, truesc): the shape is the alignment wanted, inserted bases random.
# At the default scoring truesc is min(qlen, tlen) - 4 - w2 for a first band w2 of 4 / 8 / 4 /
# 16; under `gaps` it was moved until the classifier gave the same path, and retry32 is longer:
# there bwa_gen_cigar2 caps the band at half of what the query could pay for
# (software/bwa.c:125-130), 11 for 100 bp, and a row of more than 32 columns needs 143 bp.
# cross16 / cross32 are retry16 / retry32 with the gaps placed so that, in the last try, an
# insertion's F chain runs from one pass of the row into the next (global_dp's carry_p) and a
# diagonal step takes H from the pass before (carry_h); _carries() counts both.
SHAPES = {
    "retry16": {"default": ("20M6I25M7D19M", 62), "gaps": ("20M6I25M7D19M", 58)},
    "retry32": {"default": ("30M10I35M10D25M", 88), "gaps": ("45M10I48M10D40M", 123)},
    "defer16": {"default": ("50M6I60M7D54M", 162), "gaps": ("50M6I60M7D54M", 158)},
    "defer64": {"default": ("100M20I100M20D80M", 280), "gaps": ("100M20I100M20D80M", 264)},
    "cross16": {"default": ("13M6I32M7D19M", 62), "gaps": ("20M7I12M1I20M9D12M", 60)},
    "cross32": {"default": ("30M8I20M3I17M11D22M", 88), "gaps": ("45M14I30M3I18M17D33M", 123)},
}
# what each must be, as (class, columns per try, try that defers)
WANT = {
    ("retry16", "default"): (0, [9, 17, 33], 0), ("retry16", "gaps"): (0, [9, 17, 17], 0),
    ("retry32", "default"): (1, [17, 33, 47], 0), ("retry32", "gaps"): (1, [17, 33, 35], 0),
    ("defer16", "default"): (0, [9, 17, 33], 3), ("defer16", "gaps"): (0, [9, 17, 33], 3),
    ("defer64", "default"): (2, [33, 65, 129], 2), ("defer64", "gaps"): (2, [33, 65, 73], 2),
    ("cross16", "default"): (0, [9, 17, 33], 0), ("cross16", "gaps"): (0, [9, 17, 17], 0),
    ("cross32", "default"): (1, [17, 33, 47], 0), ("cross32", "gaps"): (1, [17, 33, 35], 0),
}


def _segs(shape):
    return [(op, int(n)) for n, op in re.findall(r"(\d+)([MID])", shape)]


@functools.lru_cache(maxsize=None)
def _retry_set(scoring):
    g = T._genome()
    B = T._Builder()
    rng = np.random.default_rng(9)
    for k, name in enumerate(SHAPES):
        shape, truesc = SHAPES[name][scoring]
        for rev in (False, True):
            # (a cross shape is laid out backwards for the reverse strand, where bwa_gen_cigar2 reverses
            # both sequences: the DP meets the gaps in the order written)
            segs = _segs(shape)[::-1] if rev and name.startswith("cross") else _segs(shape)
            p = t = 17500 + 400 * k
            parts = []
            for op, n in segs:
                if op == "I":
                    parts.append(rng.integers(0, 4, n, dtype=np.uint8))
                else:
                    if op == "M":
                        parts.append(g[t:t + n])
                    t += n
            B.one(np.concatenate(parts), p, t - p, rev, truesc, 100, name + ("r" if rev else "f"),
                  clip=(3, 0) if rev else (0, 2))
    reads, regs, reg_off = B.arrays()
    return reads, regs, reg_off, tuple(B.tags)


def _carries(ops, w, G):
    """Over the path of a CIGAR (M / I / D runs in the DP's order) in a band of w on lane
    groups of G: (insertions whose F chain starts in one G-column pass of its row and ends
    in a later one, diagonal steps whose H comes from the last column of the pass before)"""
    i = j = n_p = n_h = 0
    col = lambda r, c: c - max(0, r - w)   # noqa: E731  (ksw_global2's beg, software/ksw.c:527)
    for op, n in ops:
        if op == "M":
            for _ in range(n):
                # H(i - 1, j - 1) reaches row i through the lane of (i - 1, j): the first lane of a later pass
                # takes it from carry_h
                if i >= 1 and j >= 1 and col(i - 1, j) > 0 and col(i - 1, j) % G == 0:
                    n_h += 1
                i, j = i + 1, j + 1
        elif op == "I":
            if i >= 1 and j >= 1:
                c0 = col(i - 1, j - 1)
                n_p += c0 // G != (c0 + n) // G
            j += n
        else:
            i += n
    return n_p, n_h


def _restate(opt, reads, regs, reg_off):
    """the restatement of every region, one DP per distinct (read, region) content"""
    rd = T._read_of_region(reg_off)
    pac = T._pack(T._genome())
    seen, out = {}, []
    for k in range(regs.size):
        key = (reads.read(int(rd[k])).tobytes(), regs[k].tobytes())
        if key not in seen:
            seen[key] = ref.reg2aln(opt, T.G_LEN, pac, reads.read(int(rd[k])), regs[k])
        out.append(seen[key])
    return out


@functools.lru_cache(maxsize=None)
def _retry_ref(scoring):
    reads, regs, reg_off, _tags = _retry_set(scoring)
    return _restate(OPTS[scoring], reads, regs, reg_off)


# ---- the scratch tier: more regions than blocks, slabs reused across row widths ----
# (qlen, deleted bases, first band w2, reverse strand): each a direction matrix of more than
# the scratch-tier kernel's 32 KB of LDS, so it lies in the block's slab
SLAB_SHAPES = [(400, 0, 80, False), (400, 0, 90, True), (500, 0, 70, False), (450, 3, 75, True), (600, 0, 60, False),
               (380, 0, 85, True), (420, 5, 88, False), (520, 2, 66, True), (640, 0, 58, False), (700, 0, 50, True),
               (480, 4, 72, False), (560, 0, 64, True)]
N_SLAB = 300
BIG_Q, BIG_T = 1024, 2048


@functools.lru_cache(maxsize=None)
def _slab_set():
    g = T._genome()
    B = T._Builder()
    sub = lambda s, i: (int(s[i]) + 1) & 3   # noqa: E731
    made = []
    for n, (ql, d, w2, rev) in enumerate(SLAB_SHAPES):
        p = 1500 + 800 * n
        h = ql // 2
        q = np.concatenate([g[p:p + h], g[p + h + d:p + ql + d]]).copy()
        for i in range(30 + n, ql, 83):
            q[i] = sub(q, i)
        # infer_bw (a 1, gaps 6 + 1) asks for w2 at truesc = qlen - 4 - w2 and is at least the length
        # difference; the clean read scores far above it: one try
        made.append((q, p, ql + d, rev, ql - 4 - w2, 100, f"slab{n}"))
    order = np.random.default_rng(11).integers(0, len(made), N_SLAB)
    order[:len(made)] = np.arange(len(made))          # every shape at least once
    p = 20000
    big = np.concatenate([g[p:p + BIG_Q // 2], g[p + BIG_Q // 2 + (BIG_T - BIG_Q):p + BIG_T]])
    for n, k in enumerate(order):
        if n == N_SLAB // 2:   # the widest matrix (it sets the slab stride) in the middle of the list
            B.one(big, p, BIG_T, False, BIG_Q - (6 + BIG_T - BIG_Q), 2 * BIG_T, "big")
        B.one(*made[int(k)])
    reads, regs, reg_off = B.arrays()
    return reads, regs, reg_off, tuple(B.tags)


@functools.lru_cache(maxsize=None)
def _slab_ref():
    reads, regs, reg_off, _tags = _slab_set()
    return _restate(OPTS["default"], reads, regs, reg_off)


def _big_grid(opt, regs, shapes):
    """run_g2a's scratch-tier launch (csrc/smem_gpu.cpp): (regions on it, blocks, slab stride)"""
    big = [k for k, s in enumerate(shapes) if s.cls == ref.SCRATCH_CLASS or s.defer_try]
    need = max(ref.scratch_need(opt, int(regs[k]["qe"] - regs[k]["qb"]), int(regs[k]["re"] - regs[k]["rb"])) for k in big)
    stride = max((need + 255) & ~255, 256)
    blocks = min(max(64, (256 << 20) // stride), 2048, len(big))
    return big, blocks, stride


def test_retry_and_slab_regions_hit_their_shapes():
    for scoring, o in OPTS.items():
        reads, regs, reg_off, tags = _retry_set(scoring)
        want = _retry_ref(scoring)
        assert len(tags) == 2 * len(SHAPES)
        for k, tag in enumerate(tags):
            a = want[k]
            s = ref.classify(o, regs[k], a.tries)
            cls, n_col, defer = WANT[(tag[:-1], scoring)]
            print(scoring, tag, a.tries, s, ref.cigar_str(a.cigar))
            assert a.status == 0 and a.tries == 3 and (s.cls, s.n_col, s.defer_try) == (cls, n_col, defer), (tag, a, s)
            shape = SHAPES[tag[:-1]][scoring][0]
            body = [c for c in a.cigar if c & 0xf != 3]                        # the last band held every gap
            gaps = lambda x: sorted((op, n) for op, n in x if op != "M")      # noqa: E731
            if not tag.startswith("cross"):
                assert gaps(("MID"[c & 0xf], c >> 4) for c in body) == gaps(_segs(shape)), (tag, ref.cigar_str(a.cigar))
            G = s.group
            if tag[:5] in ("retry", "cross"):   # every try in the group's LDS, rows of 2 and more passes
                assert max(s.nbytes) <= ref.group_lds(G) and s.n_col[0] <= G < s.n_col[1] and s.n_col[2] > G
            else:                         # hands over after a try of its own
                assert s.nbytes[defer - 1] > ref.group_lds(G) >= s.nbytes[defer - 2] and s.nbytes[defer - 1] <= ref.LDS_BIG
            if tag.startswith("cross"):   # the last try's path needs both carries between passes
                ql, tl = int(regs[k]["qe"] - regs[k]["qb"]), int(regs[k]["re"] - regs[k]["rb"])
                w = ref.band(o, ql, tl, ref.first_w2(o, ql, tl, int(regs[k]["truesc"]), int(regs[k]["w"])) << 2)
                path = [("MID"[c & 0xf], c >> 4) for c in body]
                n_p, n_h = _carries(path[::-1] if a.is_rev else path, w, G)
                print(scoring, tag, "band", w, "carry_p", n_p, "carry_h", n_h)
                assert min(ql, 2 * w + 1) == s.n_col[2]
                # (under `gaps` the reverse strand's restatement splits the deletion instead of paying for the
                # one-base insertion at the band's edge: that region is held to its class and tries alone)
                if not (a.is_rev and scoring == "gaps" and tag == "cross16r"):
                    assert n_p >= 1 and n_h >= 1, (tag, w, n_p, n_h)
        assert ref.classify(o, regs[tags.index("defer16f")], 3).n_col[1] > 16   # ... a multi-pass one in the 16-lane class
    # the slab set
    o = OPTS["default"]
    reads, regs, reg_off, tags = _slab_set()
    want = _slab_ref()
    shapes = [ref.classify(o, regs[k], want[k].tries) for k in range(regs.size)]
    assert all(a.status == 0 and a.tries == 1 for a in want)
    assert all(s.cls == ref.SCRATCH_CLASS and s.nbytes[0] > ref.LDS_BIG for s in shapes)   # every matrix in a slab
    big, blocks, stride = _big_grid(o, regs, shapes)
    k_big = tags.index("big")
    assert stride == BIG_Q // 2 * BIG_T == ref.row_bytes(BIG_Q, 10 ** 6) * BIG_T and blocks == 256
    assert len(big) == regs.size == N_SLAB + 1 > blocks                  # the grid loops, slabs are reused
    assert shapes[k_big].n_col == [BIG_Q] and "1024D" in ref.cigar_str(want[k_big].cigar)
    widths = {(s.n_col[0] + 1) >> 1 for s in shapes}
    assert len(widths) >= 10
    # blocks take regions it, it + blocks, ...: some slab is reused by another row width
    assert any(shapes[k].n_col != shapes[k + blocks].n_col for k in range(regs.size - blocks))
    assert len({tags[k] for k in range(12)}) == 12 and any(tags[k] != tags[k + 1] for k in range(12, 40))
    assert all("D" in ref.cigar_str(want[k].cigar) for k, t in enumerate(tags) if t != "big" and SLAB_SHAPES[int(t[4:])][1])


def _run(gpu_device, reads, regs, reg_off, opt, want, tags, what):
    gpu = T._gpu_for(T._genome(), gpu_device)
    try:
        alns, cigar, md, ms = gpu.reg2aln(T._pack(T._genome()), T.G_LEN, reads.codes, reads.offs, regs, reg_off,
                                          T._c_opt(opt))
        assert gpu.fault()[0] == 0
    finally:
        gpu.close()
    print(f"reg2aln {what}: {regs.size} regions, kernel {ms:.3f} ms")
    got = [T._got(alns, cigar, md, k) for k in range(regs.size)]
    bad = [(k, tags[k], got[k], want[k]) for k in range(regs.size) if got[k] != want[k]]
    assert not bad, (len(bad), bad[:3])
    assert int(alns["n_cigar"].sum()) == cigar.size and int(alns["md_len"].sum()) == md.size


@pytest.mark.gpu
@pytest.mark.parametrize("scoring", list(OPTS))
def test_reg2aln_gpu_retries_and_deferrals(gpu_device, scoring):
    """retry16 / retry32 / defer16 / defer64 on both strands: every field equals the
    restatement (three tries each, the gapped CIGAR of the last band)"""
    reads, regs, reg_off, tags = _retry_set(scoring)
    _run(gpu_device, reads, regs, reg_off, OPTS[scoring], _retry_ref(scoring), tags, "retries " + scoring)


@pytest.mark.gpu
def test_reg2aln_gpu_scratch_tier_reuses_slabs(gpu_device):
    """301 scratch-tier regions of 13 shapes on 256 blocks with 1 MB slabs: every field of
    every region equals the restatement"""
    reads, regs, reg_off, tags = _slab_set()
    _run(gpu_device, reads, regs, reg_off, OPTS["default"], _slab_ref(), tags, "slabs")
