"""smem_kmer_probe_depth on hand-made level tables (no GPU): the depth a bwt_smem1 call probes the k-mer
table at, from the stored levels' minimum sizes mn[1..k], the table's depth k, the smallest size of the
unstored level k + 1 (0 or 2^64 - 1: a string is absent, or the level was not reduced) and the call's
min_intv.  It is the largest level L <= k with levels 1 .. L + 1 complete and mn[L] >= min_intv: k itself
where the unstored level is complete too, smem_kmer_call_depth(mn, smem_kmer_depth(mn, k), min_intv)
otherwise (tests/test_kmer_depth.py pins those two)."""
import numpy as np

UNKNOWN = 2 ** 64 - 1
MIN_INTVS = (1, 0, -3, 9, 10, 51, 201, 901)   # the values of test_kmer_depth.py's cases


def _mn(levels):
    a = np.zeros(16, np.uint64)
    a[1:1 + len(levels)] = levels
    return a


def _probe(levels, min_next, min_intv, k=None):
    import smemgpu
    a = _mn(levels)
    return smemgpu.load().smem_kmer_probe_depth(a.ctypes.data, len(levels) if k is None else k, min_next, min_intv)


def _old(levels, min_intv, k=None):
    import smemgpu
    lib = smemgpu.load()
    a = _mn(levels)
    return lib.smem_kmer_call_depth(a.ctypes.data, lib.smem_kmer_depth(a.ctypes.data, len(levels) if k is None else k),
                                    min_intv)


def test_extra_level_complete_reaches_k():
    lv = [900, 200, 50, 9, 2]
    assert _probe(lv, 1, 1) == 5          # all five levels and the sixth complete, minsz[5] = 2 >= 1
    assert _probe(lv, 1, 2) == 5          # equal: the size may touch min_intv
    assert _probe(lv, 700, 2) == 5        # (the unstored minimum's value beyond "> 0" plays no part)
    assert _probe([900], 3, 1) == 1       # a table of one level
    assert _probe([900], 3, 900) == 1 and _probe([900], 3, 901) == 0
    assert _probe(lv, 1, 1, k=3) == 3     # judged on its k levels: level 4 is then the "unstored" one
    assert _old(lv, 1) == 4               # what the stored levels alone allow


def test_extra_level_incomplete_or_unknown_changes_nothing():
    tables = ([900, 200, 50, 9, 2], [900, 200, 50, 9, 2, 0], [900], [900, 200, 0, 0, 0], [900, 0, 0], [0, 0, 0],
              [900, 0, 50, 9])
    for lv in tables:
        for mi in MIN_INTVS:
            for nx in (0, UNKNOWN):
                assert _probe(lv, nx, mi) == _old(lv, mi), (lv, nx, mi)
    for mi in MIN_INTVS:
        for nx in (0, UNKNOWN):
            assert _probe([900, 200, 50, 9, 2], nx, mi, k=3) == _old([900, 200, 50, 9, 2], mi, k=3)


def test_min_intv_between_the_last_two_levels():
    lv = [900, 200, 50, 9, 2]
    assert _probe(lv, 1, 3) == 4          # minsz[5] = 2 < 3 <= minsz[4] = 9: k - 1
    assert _probe(lv, 1, 9) == 4
    assert _probe(lv, 1, 10) == 3
    assert _probe(lv, 1, 51) == 2
    assert _probe(lv, 1, 201) == 1
    assert _probe(lv, 1, 901) == 0


def test_gap_at_a_stored_level_is_unchanged():
    # a string of 3 bases is absent: the unstored level cannot be complete, whatever it is said to be
    for nx in (0, 1, 50, UNKNOWN):
        for mi in MIN_INTVS:
            assert _probe([900, 200, 0, 0, 0], nx, mi) == _old([900, 200, 0, 0, 0], mi)
            assert _probe([900, 200, 50, 9, 0], nx, mi) == _old([900, 200, 50, 9, 0], mi)   # the gap at level k
            assert _probe([900, 0, 50, 9], nx, mi) == _old([900, 0, 50, 9], mi)            # a level after a gap
            assert _probe([0, 0, 0], nx, mi) == 0
    assert _probe([900, 200, 50, 9, 0], 1, 1) == 3


def test_k15_is_never_15():
    lv = [10 ** 9 >> l for l in range(15)]    # 15 complete levels
    assert all(v > 0 for v in lv)
    for nx in (0, 1, 5, UNKNOWN):
        for mi in (1, 0, 2, 10 ** 9):
            assert _probe(lv, nx, mi) == _old(lv, mi) <= 14, (nx, mi)
    assert _probe(lv, 5, 1) == 14
    assert _probe(lv, 5, 1, k=14) == 14       # 14 levels and the fifteenth vouched for
    assert _probe(lv, 0, 1, k=14) == 13


def test_min_intv_at_most_zero_is_one():
    lv = [900, 200, 50, 9, 2]
    for mi in (0, -1, -3, -2 ** 40):
        assert _probe(lv, 1, mi) == _probe(lv, 1, 1) == 5
        assert _probe(lv, 0, mi) == _probe(lv, 0, 1) == 4
