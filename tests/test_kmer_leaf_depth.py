"""smem_kmer_leaf_probe_depth on hand-made level tables (no GPU): the depth a launch probes at on a table
that stores one level more than the k it reports (DESIGN.md §5 "A leaf level").  The leaf, level k + 1
(smallest size min_next), is the answer when levels 1 .. k + 1 are complete, min_next >= min_intv, and the
leaf is strict or level k + 2 (smallest size leaf_next) is complete; smem_kmer_probe_depth's answer on the
k levels otherwise, and always without a leaf (tests/test_kmer_probe_depth.py pins that function)."""
import numpy as np

UNKNOWN = 2 ** 64 - 1
MIN_INTVS = (1, 0, -3, 2, 3, 9, 10, 51, 201, 901)
LV = [900, 200, 50, 9]      # levels 1..4; the leaf is level 5


def _mn(levels, fill=0):
    a = np.full(16, fill, np.uint64)
    a[0] = 0
    a[1:1 + len(levels)] = levels
    return a


def _leaf(levels, min_next, leaf, strict, leaf_next, min_intv, k=None, fill=0):
    import smemgpu
    a = _mn(levels, fill)
    return smemgpu.load().smem_kmer_leaf_probe_depth(a.ctypes.data, len(levels) if k is None else k, min_next,
                                                     leaf, strict, leaf_next, min_intv)


def _old(levels, min_next, min_intv, k=None, fill=0):
    import smemgpu
    a = _mn(levels, fill)
    return smemgpu.load().smem_kmer_probe_depth(a.ctypes.data, len(levels) if k is None else k, min_next, min_intv)


def test_no_leaf_is_the_old_function():
    tables = (LV, LV + [0], [900], [900, 200, 0, 0], [0, 0, 0], [900, 0, 50, 9])
    for lv in tables:
        for nx in (0, 1, 2, 700, UNKNOWN):
            for mi in MIN_INTVS:
                for strict in (0, 1):
                    for ln in (0, 1, 40, UNKNOWN):     # the leaf's facts play no part without a leaf
                        assert _leaf(lv, nx, 0, strict, ln, mi) == _old(lv, nx, mi), (lv, nx, mi, strict, ln)


def test_complete_strict_and_large_enough_reaches_the_leaf():
    assert _old(LV, 2, 1) == 4
    for ln in (0, UNKNOWN, 1, 40):                     # level k + 2 may be incomplete or unknown
        assert _leaf(LV, 2, 1, 1, ln, 1) == 5
        assert _leaf(LV, 2, 1, 1, ln, 2) == 5          # equal: the size may touch min_intv
        assert _leaf(LV, 2, 1, 1, ln, 0) == 5 and _leaf(LV, 2, 1, 1, ln, -7) == 5   # min_intv < 1 taken as 1
    assert _leaf([900], 3, 1, 1, 0, 1) == 2            # a table of one level and its leaf
    assert _leaf(LV, 2, 1, 1, 0, 1, k=3) == 4          # judged on its k levels: the leaf is then level 4


def test_not_strict_needs_the_next_level_complete():
    for mi in MIN_INTVS:
        for ln in (0, UNKNOWN):
            assert _leaf(LV, 2, 1, 0, ln, mi) == _old(LV, 2, mi), (mi, ln)          # the old answer
    assert _leaf(LV, 2, 1, 0, 0, 1) == 4
    for ln in (1, 40):                                  # level k + 2 complete implies strictness
        assert _leaf(LV, 2, 1, 0, ln, 1) == 5 and _leaf(LV, 2, 1, 0, ln, 2) == 5


def test_leaf_smaller_than_min_intv_falls_back_for_that_min_intv_only():
    for strict, ln in ((1, 0), (0, 7), (1, 7)):
        assert _leaf(LV, 2, 1, strict, ln, 2) == 5
        assert _leaf(LV, 2, 1, strict, ln, 3) == _old(LV, 2, 3) == 4     # minsz[5] = 2 < 3 <= minsz[4] = 9
        assert _leaf(LV, 2, 1, strict, ln, 10) == _old(LV, 2, 10) == 3
        assert _leaf(LV, 2, 1, strict, ln, 901) == 0
        assert _leaf(LV, 2, 1, strict, ln, 1) == 5                       # ... and the smaller one still gets the leaf


def test_incomplete_leaf_or_stored_level_is_the_old_answer():
    for mi in MIN_INTVS:
        for strict in (0, 1):
            for ln in (0, 1, UNKNOWN):
                for nx in (0, UNKNOWN):                 # a string of the leaf is absent, or it was not reduced
                    assert _leaf(LV, nx, 1, strict, ln, mi) == _old(LV, nx, mi), (mi, strict, ln, nx)
                for lv in ([900, 200, 0, 0], [900, 0, 50, 9], [900, 200, 50, 0], [0, 0, 0]):   # a gap below it
                    assert _leaf(lv, 2, 1, strict, ln, mi) == _old(lv, 2, mi), (lv, mi, strict, ln)
    assert _leaf(LV, 0, 1, 1, 1, 1) == 3


def test_k14_and_k15_stay_inside_the_arrays():
    lv = [10 ** 9 >> l for l in range(15)]              # 15 complete levels
    assert all(v > 0 for v in lv)
    # k = 14: the leaf is level 15, the deepest a launch can run at; its facts come as arguments, and mn[15],
    # mn[0] and whatever lies beside the 14 levels are not read (poisoned here with 0 and with all ones)
    for fill in (0, UNKNOWN):
        assert _leaf(lv[:14], 5, 1, 1, 0, 1, fill=fill) == 15
        assert _leaf(lv[:14], 5, 1, 0, 3, 1, fill=fill) == 15
        assert _leaf(lv[:14], 5, 1, 0, 0, 1, fill=fill) == _old(lv[:14], 5, 1, fill=fill) == 14
        assert _leaf(lv[:14], 5, 1, 1, 0, 6, fill=fill) == _old(lv[:14], 5, 6, fill=fill) == 14
        assert _leaf(lv[:14], 0, 1, 1, 0, 1, fill=fill) == 13
    # k = 15: there is no level 16 to probe, whatever the leaf is said to be
    for nx in (0, 1, 5, UNKNOWN):
        for mi in (1, 0, 2, 10 ** 9):
            for strict in (0, 1):
                for ln in (0, 4, UNKNOWN):
                    assert _leaf(lv, nx, 1, strict, ln, mi) == _old(lv, nx, mi) <= 14, (nx, mi, strict, ln)
    # k out of range answers like the old function as well
    assert _leaf(lv, 5, 1, 1, 4, 1, k=0) == _old(lv, 5, 1, k=0) == 0
