// Alignments -> single-end SAM text on the device: mem_reg2sam_se (software/bwamem.c:1359-1393)
// through mem_aln2sam (:1214-1327) with extra_flag 0 and no mate, over the records
// smem_batch_reg_finalize and smem_batch_reg2aln left in HBM (or a caller's host buffers); and
// the paired-end text of mem_sam_pe's tail over a caller's host buffers (SamPeParams below).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fin_kernels.h"
#include "global_kernels.h"

namespace smem {

constexpr int SAM_HOST = 1;          // SMEM_SAM_HOST
constexpr int SAM_NAME_MAX = 255;    // bytes of a read name
// the write kernel: one wave a block, its staging window in LDS; a CIGAR batch of 64 ops
// (at most 10 digits and a letter each) must fit behind what a flush leaves (< 16 bytes)
constexpr int SAM_BUF = 2048;
// the write kernel's grid: 16 one-wave blocks a CU of 256 (its 98 VGPRs allow 20), reads taken in turn
constexpr int SAM_WRITE_BLOCKS_MAX = 4096;
static_assert(SAM_BUF % 16 == 0 && SAM_BUF >= 64 * 11 + 16, "staging window");

// what a record carries beside its smem_aln_t when the caller passes host buffers (smem_sam_rec_t)
struct SamRec {
    int32_t mapq, flag, score, xs;
};

// the device's counters of one call (u32): reads whose written bytes differ from their counted
// bytes (never expected: the host reports SMEM_E_INTERNAL), reads left to the host
constexpr int SAM_N_BADLEN = 0, SAM_N_HOST = 1, SAM_CNTS = 2;

struct SamParams {
    // the reads: codes 0..4, offs[n_reads + 1]; qual by the same offsets (nullptr: '*');
    // names / comments by their own offsets (comments nullptr: none)
    const uint8_t* codes;
    const uint64_t* offs;
    const char* qual;
    const char* names;
    const uint64_t* name_off;
    const char* comments;
    const uint64_t* comment_off;
    uint32_t n_reads, n_rec;
    // the records: read r's are [rec_off[r], rec_off[r + 1]) in list order
    const uint64_t* rec_off;
    const Aln* alns;
    const int32_t* rid;
    // either recs (host-buffer call), or the finalize stage's arrays: record k is final region idx[k]
    const SamRec* recs;
    const uint64_t* idx;
    const FinSel* sel;
    const G2aReg* regs;
    const int32_t* fin_status;  // per read or nullptr
    const uint32_t* cigar;
    const char* md;
    // bns->anns[].offset / .name
    const int64_t* ctg_off;
    const char* ctg_names;
    const uint64_t* ctg_name_off;
    int32_t n_ctg;
    const char* rg;             // bwa_rg_id, rg_len bytes (0: no RG tag)
    uint32_t rg_len;
    // the length pass: per record its bytes without SA:Z and the bytes of its entry in another
    // record's SA:Z (bit 31 of rec_len: the record sends its read to the host); per read its bytes
    uint32_t* rec_len;
    uint32_t* sa_len;
    uint64_t* read_bytes;       // [n_reads]: the offset scan's input
    int32_t* status;            // [n_reads]: 0 or SAM_HOST
    // the write pass
    const uint64_t* text_off;   // [n_reads + 1]
    char* text;
    uint32_t* cnt;              // [SAM_CNTS]
};

// ---- the paired-end text (mem_sam_pe's tail, software/bwamem_pair.c:305-331; mem_aln2sam with a
// mate, software/bwamem.c:1219-1260).  Reads 2p and 2p + 1 are pair p.
// what the stage takes from smem_pair_sel_t: mode is the branch (0..2), or -1 for a pair that
// is the host's; mapq[e] is printed in branch 1 and 2; proper is extra_flag & 2 before the AND of :321
struct SamPair {
    int32_t mode, mapq[2], proper;
};

struct SamPeParams {
    SamParams s;                // n_reads == 2 n_pairs, recs set
    const SamPair* pairs;       // [n_pairs]
    uint32_t* rlen;             // [n_rec]: get_rlen of every record's CIGAR (the length pass writes it)
};

}  // namespace smem

// the length pass: sam_len_kernel (one lane per record), then sam_read_kernel (one lane per read)
extern "C" hipError_t smem_launch_sam_len(const smem::SamParams* P, hipStream_t st);
// the write pass over text_off (the scan of read_bytes)
extern "C" hipError_t smem_launch_sam_write(const smem::SamParams* P, hipStream_t st);
// the same two passes of the paired-end text: sam_len_pe_kernel, sam_read_pe_kernel; sam_write_pe_kernel
extern "C" hipError_t smem_launch_sam_pe_len(const smem::SamPeParams* X, hipStream_t st);
extern "C" hipError_t smem_launch_sam_pe_write(const smem::SamPeParams* X, hipStream_t st);
extern "C" hipError_t smem_preload_sam(void);
