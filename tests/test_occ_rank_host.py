"""The Occ64 bucket with bit-plane symbols and the extend's two forms, on the host (DESIGN.md §5 "Bit-plane
symbols and 32-bit counts").

csrc/occ_rank.h is compiled for the CPU as well: smem_occ64_host is occ64_kernel's loop and smem_extend_host one
extend_counts64 / extend_counts32 on two caller-supplied buckets, so the arithmetic is checked here against Python
integers on counts no index a test can build reaches (headers near 2^32 and 2^33, rows past 2^32).

The model never looks at a bucket's bits: it keeps each bucket as (C, G, T before it, its 64 symbols) and counts
symbols in a list.  The buckets handed to the library are packed from that by _pack, which states the layout once
more: words 0-2 the counts' low words, word 3 their bits 32-33, words 4-5 plane L (bit i = bit 0 of symbol i),
words 6-7 plane H (bit 1).

Two choices made here:
 * "a genome whose symbol count mod 128 is 1, 63, 64 and 127": the genome's own length.  The index holds both
   strands, so the BWT's symbol count is always even; lengths that leave the BWT 2 and 126 symbols into a
   128-block (the nearest to 1 and 127 an index can be) are added to the four.
 * the 32-bit form is exact while every Occ is below 2^32 (smem_occ_narrow_ok; an index beyond it runs the 64-bit
   form).  The cases that put an Occ at or above 2^32 (headers of 2^32 - 5 plus 10, around 2^33) are outside it: there
   the 64-bit form is asserted exact, and of the 32-bit form what its arithmetic still promises: the size and the
   other side exact, the start exact mod 2^32.  The same carries are asserted exactly for it where they exist inside
   the bound: the row's low word wrapping (kk = 2^32 - 1, ll = 2^32 + 70), a count reaching 2^32 - 1, and the carry
   out of L2[c] + 1's low word.
"""
import ctypes as C

import numpy as np
import pytest

M32 = (1 << 32) - 1


@pytest.fixture(scope="module")
def lib(built):
    import smemgpu
    return smemgpu.load()


# ---------------------------------------------------------------- the model
class Bkt:
    """One bucket: (C, G, T) before it and its 64 symbols."""

    def __init__(self, hdr, syms):
        self.hdr = [int(v) for v in hdr]
        self.syms = [int(v) for v in syms]
        assert len(self.hdr) == 3 and len(self.syms) == 64

    def occ(self, row):
        """Occ(A / C / G / T) through `row` (a row of this bucket, the $ row not counted)."""
        pre = self.syms[:(row & 63) + 1]
        cgt = [self.hdr[i] + pre.count(i + 1) for i in range(3)]
        return [row + 1 - sum(cgt)] + cgt

    def whole(self):
        return [self.syms.count(c) for c in (1, 2, 3)]


def _pack(b):
    lo = sum((s & 1) << i for i, s in enumerate(b.syms))
    hi = sum((s >> 1) << i for i, s in enumerate(b.syms))
    h = b.hdr
    w3 = (h[0] >> 32) | (h[1] >> 32) << 2 | (h[2] >> 32) << 4
    assert all(v < (1 << 34) for v in h)
    return np.array([h[0] & M32, h[1] & M32, h[2] & M32, w3, lo & M32, lo >> 32, hi & M32, hi >> 32], np.uint32)


def _model(bk, bl, a, b, s, c, primary, L2):
    """bwt_extend restricted to child c (software/bwt.c:416-429), in Python integers."""
    k, l = a - 1, a - 1 + s
    kk, ll = k - (k >= primary), l - (l >= primary)
    tk, tl = bk.occ(kk), bl.occ(ll)
    d = [tl[i] - tk[i] for i in range(4)]
    assert all(v >= 0 for v in d), "the case's buckets are inconsistent"
    na = L2[c] + 1 + tk[c]
    nb = b + (1 if a <= primary <= a + s - 1 else 0) + sum(d[c + 1:])
    return (na, nb, d[c]), kk, ll, tk, tl


def _run(lib, bk, bl, a, b, s, c, primary, L2, narrow):
    k, l = a - 1, a - 1 + s
    kk, ll = k - (k >= primary), l - (l >= primary)
    wk, wl = _pack(bk), _pack(bl)
    l2 = (C.c_uint64 * 5)(*[int(v) for v in L2])
    out = (C.c_uint64 * 3)()
    rc = lib.smem_extend_host(wk.ctypes.data, wl.ctypes.data, kk, ll, a, b, s, c, primary, l2, int(narrow), out)
    assert rc == 0
    return tuple(int(v) for v in out)


def _check(lib, bk, bl, a, b, s, primary, L2, narrow_exact=True, tag=""):
    """Both forms for c = 0..3 against the model.  narrow_exact False: an Occ of the case is >= 2^32."""
    for c in range(4):
        want, kk, ll, tk, tl = _model(bk, bl, a, b, s, c, primary, L2)
        assert (kk >> 6 == ll >> 6) == (bk is bl), tag
        in_bound = max(tk + tl) <= M32 and s <= M32
        assert in_bound == narrow_exact, (tag, "the case is not on the side of the bound it was made for", tk, tl)
        assert _run(lib, bk, bl, a, b, s, c, primary, L2, 0) == want, (tag, "wide", c)
        got = _run(lib, bk, bl, a, b, s, c, primary, L2, 1)
        if narrow_exact:
            assert got == want, (tag, "narrow", c)
        else:
            assert got[1:] == want[1:] and got[0] & M32 == want[0] & M32, (tag, "narrow, outside its bound", c)


def _next_bucket(rng, bk, gap_blocks):
    """A bucket gap_blocks (>= 1) blocks after bk whose header continues bk's: the rest is random."""
    between = rng.multinomial(64 * (gap_blocks - 1), [0.25] * 4)
    hdr = [bk.hdr[i] + bk.whole()[i] + int(between[i + 1]) for i in range(3)]
    return Bkt(hdr, rng.integers(0, 4, 64))


def _bucket_at(rng, block, hdr=None, syms=None):
    """A bucket for block `block` with a header no larger than the rows before it allow."""
    if hdr is None:
        hdr = [int(v) for v in rng.multinomial(64 * block, [0.25] * 4)[1:]]
    assert sum(hdr) <= 64 * block
    return Bkt(hdr, rng.integers(0, 4, 64) if syms is None else syms)


L2_SMALL = [0, 1 << 20, 2 << 20, 3 << 20, 4 << 20]


# ---------------------------------------------------------------- counts
def _count_buckets():
    rng = np.random.default_rng(5)
    out = [("random%d" % i, rng.integers(0, 4, 64)) for i in range(6)]
    out += [("allA", np.zeros(64, int)), ("allC", np.full(64, 1)), ("allG", np.full(64, 2)), ("allT", np.full(64, 3))]
    r = [int(v) for v in rng.integers(0, 2, 64)]
    for name, bits in (("planes differ at 31 / 32 / 63", (31, 32, 63)), ("at 31", (31,)), ("at 32", (32,)), ("at 63", (63,))):
        out.append((name, [r[i] | (r[i] ^ (i in bits)) << 1 for i in range(64)]))   # L = r, H = r but for those bits
    return out


@pytest.mark.parametrize("name,syms", _count_buckets(), ids=[n for n, _ in _count_buckets()])
def test_counts_every_position(lib, name, syms):
    """Occ(c) through every position of a bucket, c = 0..3, read off the child's start (L2 = 0: na - 1)."""
    hdr = [1000, 2000, 3000]
    block = 200
    bk = Bkt(hdr, syms)
    L2 = [0, 0, 0, 0, 1 << 30]
    primary = 1 << 29     # beyond every row used: kk = k
    for pos in range(64):
        row = 64 * block + pos
        want = bk.occ(row)
        for narrow in (0, 1):
            got = [_run(lib, bk, bk, row + 1, 0, 0, c, primary, L2, narrow)[0] - 1 for c in range(4)]
            assert got == want, (name, pos, narrow)
    if name.startswith("planes"):
        w = [int(v) for v in _pack(bk)]
        assert (w[4] | w[5] << 32) ^ (w[6] | w[7] << 32) == (1 << 31 | 1 << 32 | 1 << 63)


# ---------------------------------------------------------------- packing
def _bwt_of(g):
    """The BWT of the text the index holds (both strands), the $ row removed, and that row (plain sorting)."""
    from smemgpu import synth
    t = [int(v) + 1 for v in synth.forward_reverse_text(g)] + [0]
    n = len(t)
    sa = sorted(range(n), key=lambda i: t[i:])
    col = [t[i - 1] for i in sa]
    primary = col.index(0)
    return [v - 1 for v in col if v], primary


@pytest.mark.parametrize("n", [257, 191, 192, 255, 193, 319])   # n mod 128: 1, 63, 64, 127; 2n mod 128: 2, 126
def test_occ64_host_packing(lib, n):
    import smemgpu
    g = np.random.default_rng(n).integers(0, 4, n).astype(np.uint8)
    idx, sa = smemgpu.Index.build_sa(g, sa_intv=32)
    try:
        bwt, primary = _bwt_of(g)
        assert primary == idx.primary and len(bwt) == idx.seq_len == 2 * n
        words = np.array(idx.words, np.uint32)
        n_ref = (words.size + 15) // 16
        ref = np.zeros(n_ref * 16, np.uint32)
        ref[:words.size] = words
        out = np.full(n_ref * 16, 0xDEADBEEF, np.uint32)
        assert lib.smem_occ64_host(ref.ctypes.data, n_ref, out.ctypes.data) == 0
        assert 64 * 2 * n_ref >= len(bwt)
        run = [0, 0, 0, 0]
        for b in range(2 * n_ref):
            w = [int(v) for v in out[8 * b:8 * b + 8]]
            hdr = [w[i] | ((w[3] >> (2 * i)) & 3) << 32 for i in range(3)]
            lo, hi = w[4] | w[5] << 32, w[6] | w[7] << 32
            assert w[3] >> 6 == 0
            if 64 * b <= len(bwt):   # (past the text the reference's words hold its closing counts, not symbols)
                assert hdr == run[1:], (n, b)
            for i in range(64):
                s = (lo >> i & 1) | (hi >> i & 1) << 1
                r = 64 * b + i
                # the reference's words, MSB first (software/bwt.h:71-78)
                assert s == int(ref[16 * (r >> 7) + 8 + ((r & 127) >> 4)]) >> ((~r & 15) << 1) & 3
                if r < len(bwt):
                    assert s == bwt[r], (n, r)
                    run[s] += 1
        assert [0] + list(np.cumsum(run)) == [int(v) for v in idx.L2]
    finally:
        idx.close()
        sa.close()


# ---------------------------------------------------------------- the extend
def test_extend_one_bucket_and_two(lib):
    rng = np.random.default_rng(11)
    primary = 5_000
    for it in range(60):
        block = int(rng.integers(1, 60))
        bk = _bucket_at(rng, block)
        pk = int(rng.integers(0, 63))
        pl = int(rng.integers(pk, 64))
        a = 64 * block + pk + 1 + (64 * block + pk >= primary)          # k = a - 1: row kk of block `block`
        _check(lib, bk, bk, a, int(rng.integers(1, 1 << 33)), pl - pk, primary, L2_SMALL, tag=f"one {it}")
        gap = int(rng.integers(1, 5))
        bl = _next_bucket(rng, bk, gap)
        pl = int(rng.integers(0, 64))
        _check(lib, bk, bl, a, int(rng.integers(1, 1 << 33)), 64 * gap + pl - pk, primary, L2_SMALL, tag=f"two {it}")


@pytest.mark.parametrize("base", [1 << 32, 1 << 33])
def test_extend_header_carry(lib, base):
    """Headers of base - 5 with the position adding 10: the carry out of a count's low word (into bit 33 around 2^33)."""
    primary = 7
    block = (base >> 6) + 200     # (the rows before it hold the headers: Occ(A) stays small)
    for which in range(3):   # the base whose Occ crosses
        hdr = [1000, 2000, 3000]
        hdr[which] = base - 5
        syms = [which + 1] * 10 + [0, 1, 2, 3] * 13 + [0, 0]
        bk = _bucket_at(None, block, hdr, syms)
        a = 64 * block + 9 + 2     # kk = 64 block + 9: ten symbols of `which` counted (k >= primary: kk = k - 1)
        _check(lib, bk, bk, a, 12345, 30, primary, L2_SMALL, narrow_exact=False, tag=f"carry {base} {which} same")
        bl = _next_bucket(np.random.default_rng(which), bk, 2)
        _check(lib, bk, bl, a, 12345, 64 * 2 + 11, primary, L2_SMALL, narrow_exact=False, tag=f"carry {base} {which} two")
        # k before the crossing, l after it
        a = 64 * block + 2 + 2
        _check(lib, bk, bk, a, 1, 20, primary, L2_SMALL, narrow_exact=False, tag=f"carry {base} {which} across")


def test_extend_counts_up_to_the_bound(lib):
    """Inside the 32-bit form's bound: a count that reaches 2^32 - 1 exactly, and headers just below it."""
    primary = 7
    block = (1 << 26) + 200
    for which in range(3):
        hdr = [1000, 2000, 3000]
        hdr[which] = (1 << 32) - 11
        syms = [which + 1] * 10 + [0] * 54
        bk = _bucket_at(None, block, hdr, syms)
        _check(lib, bk, bk, 64 * block + 2, 99, 9, primary, L2_SMALL, tag=f"bound {which}")   # Occ(l) = 2^32 - 1
    hdr = [(1 << 32) - 70] * 3                      # all three large at once
    bk = _bucket_at(np.random.default_rng(3), 3 << 26, hdr)
    _check(lib, bk, bk, 64 * (3 << 26) + 3, 1 << 33, 58, primary, L2_SMALL, tag="bound all")


def test_extend_rows_across_2_32(lib):
    """kk = 2^32 - 1 with ll = 2^32 + 70: the rows' low words wrap between k and l."""
    rng = np.random.default_rng(21)
    primary = 100
    kk, ll = (1 << 32) - 1, (1 << 32) + 70
    bk = _bucket_at(rng, kk >> 6, [1 << 30, (1 << 30) + 5, (1 << 30) - 9])
    bl = _next_bucket(rng, bk, 2)
    assert (ll >> 6) - (kk >> 6) == 2
    a = kk + 2     # k = kk + 1 (past primary)
    _check(lib, bk, bl, a, 3 << 30, ll - kk, primary, [0, 1 << 30, 2 << 30, 3 << 30, 1 << 33], tag="rows across 2^32")


def test_extend_size_2_32_minus_1(lib):
    rng = np.random.default_rng(22)
    primary = 3
    s = (1 << 32) - 1
    kk = 64 * 1000 + 17
    ll = kk + s
    bk = _bucket_at(rng, kk >> 6)
    bl = _next_bucket(rng, bk, (ll >> 6) - (kk >> 6))
    _check(lib, bk, bl, kk + 2, 77, s, primary, [0, 1 << 31, 3 << 31, 5 << 31, 6 << 31], tag="size 2^32 - 1")
    # all of it one base, none of that base before it: that child's size is 2^32 - 1 (its Occ at l too), the others' 0
    for which in range(4):
        other = (which + 1) & 3
        pre = (kk & 63) + 1
        hdr = [0, 0, 0]
        if other:
            hdr[other - 1] = 64 * (kk >> 6)        # every row before the bucket holds `other`
        bk = Bkt(hdr, [other] * pre + [which] * (64 - pre))
        hdr = [hdr[i] + bk.whole()[i] for i in range(3)]
        if which:
            hdr[which - 1] += s - (64 - pre) - ((ll & 63) + 1)    # the blocks between the two
        bl = Bkt(hdr, [which] * 64)
        _check(lib, bk, bl, kk + 2, 77, s, primary, [0, 1 << 31, 3 << 31, 5 << 31, 6 << 31], tag=f"size, all {which}")
        assert _model(bk, bl, kk + 2, 77, s, which, primary, [0] * 5)[0][2] == s


def test_extend_around_primary(lib):
    """The interval containing primary, ending one row before it, starting one row after it: the $ in nb, and the
    rows kk / ll shifted past it."""
    rng = np.random.default_rng(23)
    block = 40
    bk = _bucket_at(rng, block)
    bl = _next_bucket(rng, bk, 1)
    primary = 64 * block + 50
    cases = {
        "contains": (primary - 10, 30),            # a <= primary <= a + s - 1
        "contains, primary first": (primary, 5),
        "contains, primary last": (primary - 4, 5),
        "ends one row before": (primary - 20, 20),   # a + s - 1 = primary - 1
        "starts one row after": (primary + 1, 20),   # a = primary + 1
    }
    flags = []
    for tag, (a, s) in cases.items():
        k, l = a - 1, a - 1 + s
        two = (k - (k >= primary)) >> 6 != (l - (l >= primary)) >> 6
        _check(lib, bk, bl if two else bk, a, 1000, s, primary, L2_SMALL, tag=tag)
        flags.append(_model(bk, bl if two else bk, a, 0, s, 3, primary, L2_SMALL)[0][1])   # c = 3: nb = b + the flag
    assert flags == [1, 1, 1, 0, 0]


def test_extend_carry_into_the_start(lib):
    """L2[c] + 1 with a low word of 0xFFFFFFF0: the add of Occ(c, k) carries into the child's high word."""
    rng = np.random.default_rng(24)
    block = 5000
    bk = _bucket_at(rng, block)
    for c in range(4):
        L2 = [0, 1 << 33, (1 << 33) + (1 << 31), (1 << 33) + (1 << 32), 3 << 32]
        L2[c] = (L2[c] & ~M32 | 0xFFFFFFF0) - 1 if c else 0xFFFFFFF0 - 1
        L2[4] = max(L2) + (1 << 31)
        assert (L2[c] + 1) & M32 == 0xFFFFFFF0
        _check(lib, bk, bk, 64 * block + 12, 5, 40, 3, L2, tag=f"start carry {c}")
        want = _model(bk, bk, 64 * block + 12, 5, 40, c, 3, L2)[0][0]
        assert want >> 32 == ((L2[c] + 1) >> 32) + 1


def test_wide_and_narrow_agree_at_random(lib):
    """Random cases inside the bound: counts up to 2^32 - 1, rows up to 6.2 G."""
    rng = np.random.default_rng(31)
    L2 = [0, 1_550_000_000, 3_100_000_000, 4_650_000_000, 6_200_000_000]
    for it in range(300):
        block = int(rng.integers(1 << 20, 6_200_000_000 >> 6))
        cap = min(M32 - 64 * 70, 64 * block // 3)
        hdr = [int(rng.integers(0, cap)) for _ in range(3)]
        bk = _bucket_at(rng, block, hdr)
        if 64 * block + 63 - sum(hdr) > M32 - 64 * 70:      # Occ(A) has to stay inside the bound too
            continue
        gap = int(rng.integers(0, 64))
        bl = _next_bucket(rng, bk, gap) if gap else bk
        pk = int(rng.integers(0, 64))
        pl = int(rng.integers(pk if not gap else 0, 64))
        primary = int(rng.integers(0, 6_200_000_000))
        kk, ll = 64 * block + pk, 64 * (block + gap) + pl
        k = kk + (kk >= primary)
        l = ll + (ll >= primary)
        if (l - (l >= primary)) != ll or (k - (k >= primary)) != kk:
            continue
        _check(lib, bk, bl, k + 1, int(rng.integers(1, 1 << 33)), l - k, primary, L2, tag=f"random {it}")


# ---------------------------------------------------------------- the rule
def test_narrow_rule(lib):
    def ok(counts):
        l2 = (C.c_uint64 * 5)(*[int(v) for v in np.concatenate([[0], np.cumsum(counts)])])
        return lib.smem_occ_narrow_ok(l2)

    assert ok([M32, 5, 5, 5]) == 1 and ok([5, 5, 5, M32]) == 1
    assert ok([M32 + 1, 5, 5, 5]) == 0 and ok([5, 5, M32 + 1, 5]) == 0 and ok([5, 5, 5, M32 + 1]) == 0
    assert ok([0, 5, 0, 5]) == 1 and ok([0, 0, 0, 0]) == 1
    assert ok([M32, M32, M32, M32]) == 1                        # all four large: 2^34 - 4 symbols
    assert ok([M32, M32, M32 + 1, M32]) == 0
    assert ok([1_550_000_000] * 4) == 1                          # a human genome's two strands
