"""Python restatement of the contig lookup around mem_reg2aln: bns_depos,
bns_pos2rid and the test at the head of bwa_fix_xref2 that decides whether a
region has to be repaired because it bridges a contig boundary.  Line numbers
cite the reference's software/ directory.  tests/test_xref_lookup.py pins it to
the reference's own records; tests/test_gpu_batch_reg2aln.py then uses it (with
tests/regfin_ref.py and tests/reg2aln_ref.py) as the expectation for
smem_batch_reg2aln."""
import functools

import numpy as np

XREF = 4                                     # SMEM_ALN_XREF


def depos(l_pac, pos):                       # bntseq.h: bns_depos
    """(forward-strand coordinate, is_rev) of a position in doubled coordinates"""
    is_rev = pos >= l_pac
    return ((l_pac << 1) - 1 - pos if is_rev else pos), int(is_rev)


def pos2rid(offsets, l_pac, pos_f):          # bntseq.c:316-330
    """the contig of forward-strand position pos_f: the reference's binary search
    over anns[].offset, -1 past the end"""
    n_seqs = len(offsets)
    if pos_f >= l_pac:                       # :319
        return -1
    left, mid, right = 0, 0, n_seqs          # :320
    while left < right:                      # :321
        mid = (left + right) >> 1
        if pos_f >= offsets[mid]:            # :323
            if mid == n_seqs - 1:            # :324
                break
            if pos_f < offsets[mid + 1]:     # :325 bracketed
                break
            left = mid + 1
        else:
            right = mid                      # :327
    return mid


def needs_fix(offsets, lens, l_pac, rb, re):  # bwa.c:195-199
    """whether bwa_fix_xref2 changes the region [rb, re) (doubled coordinates, within
    one strand): the contig of its middle point does not hold all of it"""
    fm, is_rev = depos(l_pac, (rb + re) >> 1)                    # :195
    rid = pos2rid(offsets, l_pac, fm)                            # :196
    off, ln = int(offsets[rid]), int(lens[rid])
    cb = (l_pac << 1) - (off + ln) if is_rev else off            # :197
    ce = cb + ln                                                 # :198
    return cb > rb or ce < re                                    # :199


def table(contigs):
    """regfin_data.contigs' [(name, offset, length)] -> (names, offsets, lengths)"""
    return ([c[0] for c in contigs], np.array([c[1] for c in contigs], dtype=np.int64),
            np.array([c[2] for c in contigs], dtype=np.int32))


@functools.lru_cache(maxsize=None)
def reads_of(name):
    """the reads a regfin_data set was made over"""
    from tests import golden_data
    if name.startswith("cigar_"):
        import test_reg2aln
        return test_reg2aln._fixture(name[6:])["reads"]
    return golden_data.aln_reads(next(f for f in golden_data.aln_fixtures() if f["file"] == name + ".smrg.gz"))


def aligned_rows(fin_rows, l_pac, pac, reads, opt=None, align=None):
    """reg2aln_ref.reg2aln under scoring `opt` over every selected final region of
    finalize()'s per-read output (a, sel, idx): per read a list of (final region, Aln) in
    selection order.  align(r, region) replaces the plain call (a caller's cache)."""
    import reg2aln_ref
    opt = opt or reg2aln_ref.Opt()
    if align is None:
        def align(r, p):
            return reg2aln_ref.reg2aln(opt, l_pac, pac, reads.read(r), p)
    return [[(a[k], align(r, a[k])) for k in idx] for r, (a, _sel, idx) in enumerate(fin_rows)]


def expected_rows(rows, contigs, l_pac, with_contigs=True):
    """aligned_rows' output with the contig lookup applied: per read a list of (final
    region, reg2aln_ref.Aln, rid); a region that needs bwa_fix_xref2 carries
    Aln(status=XREF) and rid -1.  Without contigs nothing is marked and every rid is -1."""
    import reg2aln_ref
    _names, offs, lens = table(contigs)
    out = []
    for row in rows:
        got = []
        for p, aln in row:
            rid = -1
            if with_contigs and aln.status in (0, reg2aln_ref.REJECT):
                if needs_fix(offs, lens, l_pac, p["rb"], p["re"]):
                    aln = reg2aln_ref.Aln(status=XREF)
                elif aln.status == 0:
                    rid = pos2rid(offs, l_pac, aln.pos)
            got.append((p, aln, rid))
        out.append(got)
    return out


@functools.lru_cache(maxsize=None)
def _aligned(name):
    """aligned_rows over a regfin_data set at the default options (computed once)"""
    import regfin_data as D
    from tests import golden_data
    F = D.load(name)
    return aligned_rows(D.restated(name)[0], F["l_pac"], golden_data.pac(F["g"]), reads_of(name))


def expected(name, with_contigs=True):
    """what smem_batch_reg2aln gives for the selection of regfin_data set `name` at the
    default options (expected_rows)"""
    import regfin_data as D
    F = D.load(name)
    return expected_rows(_aligned(name), F["contigs"], F["l_pac"], with_contigs)
