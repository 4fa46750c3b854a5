"""The single-end SAM text restated (tests/samtext_ref.py: mem_reg2sam_se through
mem_aln2sam, software/bwamem.c:1214-1393) against the reference's own lines, byte for byte,
without a GPU; and the library's new entry points as far as they go without a device.

The restatement runs over the committed raw regions (tests/regfin_ref.py, tests/reg2aln_ref.py,
tests/xref_ref.py produce the records).  Whole lines are compared, not fields: on the golden
single-end reads (sam/g1_se.sam.gz, sam/g2_se.sam.gz: one record a read, one quality character)
and on the two files of tests/golden/samtext/ (split alignments: SA:Z, hard clips, trimmed and
reversed SEQ / QUAL with qualities that are neither constant nor palindromic, names of 2 to 19
bytes, unmapped lines).

A read the stage leaves to the host (SMEM_SAM_HOST: here always a record bridging two contigs,
SMEM_ALN_XREF, which bwa_fix_xref2 would repair) has no text to compare; the reads left out
must be exactly the ones pinned in samtext_data.HOST_READS and at most 1 % of a set, so that
the comparison cannot pass by skipping.

RG:Z, comments, MEM_F_ALL secondaries (`*\\t*`, no SA:Z) and MEM_F_NO_MULTI (0x10000 printed as
0x100) cannot be pinned to the compiled reference: `ref_harness mem` takes only -k -w -A -B -d
-O -E -L and drops the FASTQ comments.  Their tests below rest on the restatement's reading of
software/bwamem.c:1264-1265, 1303, 1325 and 1233.
"""
import ctypes as C
import re

import numpy as np
import pytest

import samtext_data as SD
import samtext_ref as S

# what the new fixtures reach (measured with the restatements; the test checks it)
REACH = {"g1_r3_default": dict(reads=548, records=654, multi=109, max_records=3, supplementary=111, no_record=5),
         "g2_r4_default": dict(reads=283, records=342, multi=59, max_records=2, supplementary=59, no_record=0)}


def _host(name):
    return [r for r, t in enumerate(SD.texts(name)) if t is None]


@pytest.mark.parametrize("name", SD.SETS)
def test_restatement_equals_the_references_lines(name):
    F, texts = SD.load(name), SD.texts(name)
    host = _host(name)
    seen = [r for r in range(len(texts)) if F["golden"][r] is not None]
    assert len(host) <= SD.HOST_CAP * len(texts), (name, host)
    n = 0
    for r in seen:
        if texts[r] is None:
            continue
        assert texts[r] == F["golden"][r], (name, r, texts[r], F["golden"][r])
        n += 1
    assert n == len(seen) - len([r for r in host if F["golden"][r] is not None]) and n >= 0.99 * len(seen)


@pytest.mark.parametrize("name", SD.NEW_SETS)
def test_new_fixture_reach_and_host_reads(name):
    """the split alignments the committed single-end SAM lacks, and the reads left to the host"""
    F, recs, texts = SD.load(name), SD.records(name), SD.texts(name)
    got = dict(reads=len(recs), records=sum(len(x) for x in recs), multi=sum(len(x) > 1 for x in recs),
               max_records=max(len(x) for x in recs), supplementary=sum(1 for x in recs for y in x if y.flag & 0x800),
               no_record=sum(1 for x in recs if not x))
    assert got == REACH[name]
    host = _host(name)
    assert host == SD.HOST_READS[name] and len(host) <= SD.HOST_CAP * len(recs)
    for r in host:                                                    # each for a record that bridges two contigs
        assert any(y.status == 4 for y in recs[r]) and all(y.status in (0, 4) for y in recs[r])
    body = b"".join(t for t in texts if t is not None)
    assert body.count(b"\tSA:Z:") == sum(len(x) for r, x in enumerate(recs) if len(x) > 1 and r not in host)
    lines = body.split(b"\n")[:-1]
    hard = [l for l in lines if b"H" in l.split(b"\t")[5]]
    assert len(hard) >= REACH[name]["supplementary"] - 4 and all(int(l.split(b"\t")[1]) & 0x800 for l in hard)
    # the trimmed SEQ of a hard-clipped line is as long as its CIGAR's query span, and QUAL as SEQ
    for l in hard:
        f = l.split(b"\t")
        span = sum(int(n) for n, op in re.findall(rb"(\d+)([MIDSH])", f[5]) if op in b"MIS")
        assert len(f[9]) == len(f[10]) == span
    rev = [l for l in lines if int(l.split(b"\t")[1]) & 0x10]
    assert len(rev) > 50 and len({len(l.split(b"\t")[0]) for l in lines}) >= 10   # both strands, many name lengths
    assert sum(1 for l in lines if int(l.split(b"\t")[1]) & 4) == REACH[name]["no_record"]


def _synthetic():
    """one read, three records: a primary, a 0x100 secondary, a supplementary on the other strand"""
    codes = np.array([0, 1, 2, 3, 4, 0, 1, 2, 3, 0], dtype=np.uint8)
    qual = np.arange(40, 50, dtype=np.uint8)
    recs = [S.Rec(rid=0, pos=104, is_rev=0, cigar=(6 << 4, 4 << 4 | 3), NM=1, md="3A2", mapq=60, flag=0, score=6, xs=3),
            S.Rec(rid=1, pos=1000, is_rev=0, cigar=(10 << 4,), NM=0, md="10", mapq=0, flag=0x100, score=10, xs=-1),
            S.Rec(rid=1, pos=1010, is_rev=1, cigar=(3 << 4 | 3, 3 << 4, 1 << 4 | 1, 3 << 4), NM=2, md="6", mapq=17,
                  flag=0x800, score=4, xs=0)]
    return codes, qual, recs, ["chrA", "chrB"], [100, 900]


def test_options_the_reference_binary_cannot_reach():
    """RG:Z, a comment, a 0x100 record between primaries, 0x10000: the restatement's reading"""
    codes, qual, recs, names, offs = _synthetic()
    t = S.read_text("q1", codes, qual, "BC:Z:x y", names, offs, recs, rg_id="grp").split(b"\n")
    assert t[0] == (b"q1\t0\tchrA\t5\t60\t6M4S\t*\t0\t0\tACGTNACGTA\t()*+,-./01\tNM:i:1\tMD:Z:3A2\tAS:i:6\tXS:i:3"
                    b"\tRG:Z:grp\tSA:Z:chrB,111,-,3S3M1I3M,17,2;\tBC:Z:x y")
    assert t[1] == b"q1\t256\tchrB\t101\t0\t10M\t*\t0\t0\t*\t*\tNM:i:0\tMD:Z:10\tAS:i:10\tRG:Z:grp\tBC:Z:x y"
    # reverse strand, which = 2: cigar[0] trims the read's end; the read reversed and complemented
    assert t[2] == (b"q1\t2064\tchrB\t111\t17\t3H3M1I3M\t*\t0\t0\tGTNACGT\t.-,+*)(\tNM:i:2\tMD:Z:6\tAS:i:4\tXS:i:0"
                    b"\tRG:Z:grp\tSA:Z:chrA,5,+,6M4S,60,1;\tBC:Z:x y")
    recs[2].flag = 0x10000                                            # MEM_F_NO_MULTI: printed as 0x100 | 0x10
    t = S.read_text("q1", codes, None, None, names, offs, recs).split(b"\n")
    assert t[2].startswith(b"q1\t272\tchrB\t111\t17\t3H3M1I3M\t*\t0\t0\tGTNACGT\t*\tNM:i:2") and b"SA:Z:chrA" in t[2]
    assert S.read_text("q2", codes, qual, None, names, offs, []) == \
        b"q2\t4\t*\t0\t0\t*\t*\t0\t0\tACGTNACGTA\t()*+,-./01\tAS:i:0\tXS:i:0\n"
    for bad in (dict(status=4), dict(mapq=-1)):
        r2 = [S.Rec(**{**recs[0].__dict__, **bad})] + recs[1:]
        assert S.read_text("q1", codes, qual, None, names, offs, r2) is None
    assert S.read_text("q1", codes, qual, None, names, offs, recs, fin_status=1) is None
    assert S.read_text("q1", codes[:0], qual[:0], None, names, offs, []) is None


def test_library_exports_and_host_side_checks(built):
    """the new symbols, constants and the statistics' layout; smem_sam_text refuses gpu == NULL
    and malformed offsets with SMEM_E_ARG before it touches a device (none is needed here)"""
    import smemgpu
    from smemgpu import lib as L
    lib = smemgpu.load()
    for sym in ("smem_gpu_load_contig_names", "smem_batch_set_read_text", "smem_batch_sam", "smem_batch_sam_results",
                "smem_batch_sam_stats", "smem_sam_text"):
        assert sym in L.EXPORTED and hasattr(lib, sym), sym
    assert L.FETCH_SAM == 64 and L.FETCH_ALL == 15 and L.SAM_HOST == 1
    # the stage's statistics have their own struct; smem_batch_stats_t ends where it ended
    assert [k for k, _ in L.SamStats._fields_] == ["sam_ms", "n_sam_bytes", "n_sam_host", "sam_write_ms"]
    assert C.sizeof(L.SamStats) == 32 and L.BatchStats._fields_[-1][0] == "n_g2a_passes"
    st = L.SamStats(1.0, 1, 1, 1.0)
    assert lib.smem_batch_sam_stats(None, C.byref(st)) == -1
    n = 2
    codes = np.zeros(20, np.uint8)
    offs = np.array([0, 10, 20], np.uint64)
    nm, nm_off = L.pack_strings(["a", "bc"])
    aln_off = np.zeros(n + 1, np.uint64)
    text = np.zeros(256, np.uint8)
    text_off = np.zeros(n + 1, np.uint64)
    status = np.zeros(n, np.int32)
    nb = C.c_uint64()
    opt = L.SamOptT(None)

    def call(gpu, offs=offs, nm_off=nm_off, aln_off=aln_off, codes=codes):
        return lib.smem_sam_text(gpu, n, codes.ctypes.data, offs.ctypes.data, nm.ctypes.data, nm_off.ctypes.data, None,
                                 None, None, aln_off.ctypes.data, None, None, None, None, None, 0, None, 0, 0, None, None,
                                 None, C.byref(opt), text.ctypes.data, text.size, text_off.ctypes.data,
                                 status.ctypes.data, C.byref(nb), None)
    assert call(None) == -1                                           # SMEM_E_ARG
    # a handle that is never dereferenced: the offsets are refused first
    fake = C.create_string_buffer(4096)
    gpu = C.cast(fake, C.c_void_p)
    assert call(gpu, offs=np.array([0, 10, 5], np.uint64)) == -1
    assert call(gpu, nm_off=np.array([0, 2, 1], np.uint64)) == -1
    assert call(gpu, nm_off=np.array([0, 1, 300], np.uint64)) == -1   # a name of more than 255 bytes
    assert call(gpu, aln_off=np.array([0, 2, 1], np.uint64)) == -1
    assert call(gpu, aln_off=np.array([1, 1, 1], np.uint64)) == -1
    assert call(gpu, aln_off=np.array([0, 1, 1], np.uint64)) == -1    # records without their arrays
    assert call(gpu, codes=np.full(20, 5, np.uint8)) == -1
    assert b"smem_sam_text" in lib.smem_strerror(-1)
