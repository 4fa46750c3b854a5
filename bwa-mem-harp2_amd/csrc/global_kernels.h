// Regions -> alignments on the device: mem_reg2aln's alignment part
// (software/bwamem.c:1504-1547) -- infer_bw, the band-doubling loop over
// bwa_gen_cigar2 (software/bwa.c:96-179) with ksw_global2 (software/ksw.c:501-584)
// and its traceback, NM / MD, the edge-deletion squeeze and the clips.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace smem {

constexpr int G2A_MAX_QLEN = 1024;  // qe - qb
constexpr int G2A_MAX_TLEN = 2048;  // re - rb
// status values of smem_aln_t (include/smem_gpu.h); DEFERRED is internal: the
// region's matrix did not fit its lane group's LDS, the scratch-tier launch redoes it
constexpr int G2A_OK = 0, G2A_UNMAPPED = 1, G2A_NOCIGAR = 2, G2A_REJECT = 3, G2A_XREF = 4, G2A_DEFERRED = 100;
constexpr int G2A_BADTRACE = 101;  // a guard tripped (never expected): the host reports SMEM_E_INTERNAL
// LDS of one region in the lane-group kernels (16 / 32 / 64 lanes: 4 / 2 / 1 regions a
// wave, so 16 / 8 / 8 KB a wave) and in the scratch-tier kernel (one region per wave)
__host__ __device__ constexpr int g2a_group_lds(int group) { return group == 64 ? 8192 : 4096; }
constexpr int G2A_LDS_BIG = 32768;
// scratch-tier grid: one scratch slab per block, as many blocks as G2A_BIG_SCRATCH holds
constexpr int G2A_BIG_BLOCKS_MIN = 64, G2A_BIG_BLOCKS_MAX = 2048;
constexpr uint64_t G2A_BIG_SCRATCH = 256ull << 20;
// lane-group launches: the grid comes from the host's upper bound of the list's length (the
// length itself stays on the device), capped; a block past the list's end leaves at once
constexpr int G2A_GRID_MAX = 1 << 16;

// smem_aln_t (include/smem_gpu.h)
struct Aln {
    int64_t pos;
    int32_t is_rev, n_cigar, NM, score, tries, status;
    uint64_t cigar_off, md_off;
    int32_t md_len, pad;
};

// mem_alnreg_t as smem_alnreg_t lays it out (include/smem_gpu.h; aln_kernels.h's AlnReg)
struct G2aReg {
    int64_t rb, re;
    int32_t qb, qe, score, truesc, sub, csub, sub_n, w, seedcov, secondary;
    uint64_t hash;
};

// one region as g2a_prep_kernel prepared it (bounds checked there); record k's task is task[k]
struct G2aTask {
    uint64_t q_off;     // codes[q_off .. q_off + qlen): the read's [qb, qe)
    int64_t rb, re;     // doubled coordinates, within one strand, 0 < re - rb <= G2A_MAX_TLEN
    int32_t qlen;       // qe - qb, 1 .. G2A_MAX_QLEN
    int32_t qb, l_query;
    int32_t truesc, w;  // mem_alnreg_t.truesc / .w
    uint32_t out;       // index into alns[]
};

// the device's counters of one pass (u32): the three lane-group lists' lengths, the scratch-tier
// list's (regions classed there by the prep kernel, then the deferred ones), regions that need
// bwa_fix_xref2, selection indices outside their read's range, guards tripped
constexpr int G2A_N_LIST0 = 0, G2A_N_BIG = 3, G2A_N_XREF = 4, G2A_N_BADIDX = 5, G2A_N_BADTRACE = 6, G2A_CNTS = 8;

// bns->anns[].offset / .len (software/bntseq.h) on the device; off == nullptr: no table
struct G2aContigs {
    const int64_t* off;
    const int32_t* len;
    int32_t n;
};

// bns_pos2rid (software/bntseq.c:316-330), the same binary search
__host__ __device__ inline int g2a_pos2rid(const int64_t* off, int n_seqs, int64_t l_pac, int64_t pos_f) {
    if (pos_f >= l_pac) return -1;
    int left = 0, mid = 0, right = n_seqs;
    while (left < right) {
        mid = (left + right) >> 1;
        if (pos_f >= off[mid]) {
            if (mid == n_seqs - 1) break;
            if (pos_f < off[mid + 1]) break;
            left = mid + 1;
        } else right = mid;
    }
    return mid;
}

// g2a_prep_kernel: one lane per record k of the selection.  Record k is regs[idx ? idx[k] : k]
// of the read r with rec_off[r] <= k < rec_off[r + 1].
struct G2aPrepParams {
    const G2aReg* regs;
    const uint64_t* idx;        // nullptr: the records are the regions, in order
    const uint64_t* rec_off;    // [n_reads + 1]
    const uint64_t* reg_range;  // [n_reads + 1]: idx[k] must lie in its read's [reg_range[r], reg_range[r + 1]);
                                // nullptr: not checked
    const uint64_t* offs;       // [n_reads + 1]: the reads in codes
    uint32_t n_reads, n_rec;
    int64_t l_pac;
    G2aContigs ctg;
    int a0, o_del, e_del, o_ins, e_ins, a, w;  // a0: mat[0]
    G2aTask* task;              // [n_rec]
    uint32_t* list;             // 4 lists of n_rec entries: 16, 32, 64 lanes; scratch tier
    uint32_t* cnt;              // [G2A_CNTS]
    unsigned long long* cur;    // G2aParams::cur ([3]: the scratch need of the regions classed for that tier)
    Aln* alns;                  // [n_rec]: settled here for every record that gets no task
    int32_t* rid;               // [n_rec] or nullptr: -1 here, the aligned records' by the DP kernels
};

struct G2aParams {
    const G2aTask* task;
    const uint32_t* list;  // task indices of this launch
    const uint32_t* n_dev; // their count, in device memory (the prep kernel's or the deferred list's)
    uint32_t n;            // the host's upper bound of *n_dev: sizes the grid
    const uint8_t* codes;
    const uint8_t* pac;
    int64_t l_pac;
    int8_t mat[28];
    int o_del, e_del, o_ins, e_ins, a, w;
    Aln* alns;
    uint32_t* cigar;       // pool of cigar_cap words
    char* md;              // pool of md_cap bytes
    uint64_t cigar_cap, md_cap;
    // [0] cigar words claimed, [1] md bytes claimed, [2] regions deferred, [3] the widest direction
    // matrix (bytes) a region of the scratch tier's list needs
    unsigned long long* cur;
    uint32_t* cnt;         // [G2A_CNTS]
    uint32_t* defer;       // the scratch tier's list: a deferred region appends itself (defer_cap entries)
    uint32_t defer_cap;
    G2aContigs ctg;
    int32_t* rid;          // [.] or nullptr: bns_pos2rid of each aligned record's final pos
    uint8_t* scratch;      // scratch tier: scratch_stride bytes per block
    uint64_t scratch_stride;
};

// infer_bw (software/bwamem.c:1194-1201)
__host__ __device__ inline int g2a_infer_bw(int l1, int l2, int score, int a, int q, int r) {
    if (l1 == l2 && l1 * a - score < (q + r - a) << 1) return 0;
    int w = (int)((double)((l1 < l2 ? l1 : l2) * a - score - q) / r + 2.);
    const int d = l1 < l2 ? l2 - l1 : l1 - l2;
    if (w < d) w = d;
    return w;
}
// the first band mem_reg2aln asks for (software/bwamem.c:1504-1508)
__host__ __device__ inline int g2a_first_w2(int qlen, int tlen, int truesc, int a, int o_del, int e_del, int o_ins,
                                            int e_ins, int opt_w, int reg_w) {
    const int tmp = g2a_infer_bw(qlen, tlen, truesc, a, o_del, e_del);
    int w2 = g2a_infer_bw(qlen, tlen, truesc, a, o_ins, e_ins);
    w2 = w2 > tmp ? w2 : tmp;
    if (w2 > opt_w) w2 = w2 < reg_w ? w2 : reg_w;
    return w2;
}
// the band bwa_gen_cigar2 gives ksw_global2 (software/bwa.c:125-132)
__host__ __device__ inline int g2a_band(int qlen, int tlen, int a0, int o_del, int e_del, int o_ins, int e_ins,
                                        int w_) {
    const int max_ins = (int)((double)(((qlen + 1) >> 1) * a0 - o_ins) / e_ins + 1.);
    const int max_del = (int)((double)(((qlen + 1) >> 1) * a0 - o_del) / e_del + 1.);
    int max_gap = max_ins > max_del ? max_ins : max_del;
    max_gap = max_gap > 1 ? max_gap : 1;
    const int d = tlen > qlen ? tlen - qlen : qlen - tlen;
    int w = (max_gap + d + 1) >> 1;
    w = w < w_ ? w : w_;
    const int min_w = d + 3;
    return w > min_w ? w : min_w;
}
// bytes of a direction-matrix row (4 bits per cell) and of the per-region LDS
// before the matrix: the column array, the query and the target
__host__ __device__ inline int g2a_row_bytes(int qlen, int w) {
    const int n_col = qlen < 2 * w + 1 ? qlen : 2 * w + 1;
    return (n_col + 1) >> 1;
}
__host__ __device__ inline int g2a_fixed_bytes(int qlen, int tlen) {
    return (qlen + 1) * 8 + ((qlen + 3) & ~3) + ((tlen + 3) & ~3);
}
// the widest direction matrix a region may need over its tries (the band uncapped)
__host__ __device__ inline uint64_t g2a_scratch_need(int qlen, int tlen, int a0, int o_del, int e_del, int o_ins,
                                                     int e_ins) {
    const int w = g2a_band(qlen, tlen, a0, o_del, e_del, o_ins, e_ins, INT32_MAX);
    return (uint64_t)g2a_row_bytes(qlen, w) * (uint64_t)tlen;
}

}  // namespace smem

// settle or classify every record, fill the tasks and the four lists (order within a list unspecified)
extern "C" hipError_t smem_launch_g2a_prep(const smem::G2aPrepParams* P, hipStream_t st);
// regions of `P->list` on lane groups of `group` (16, 32 or 64) lanes, matrix in LDS;
// a region whose matrix does not fit is marked G2A_DEFERRED, counted in cur[2] and appended to `defer`
extern "C" hipError_t smem_launch_g2a(const smem::G2aParams* P, int group, hipStream_t st);
// one region per wave on `blocks` blocks, matrix in LDS when it fits, else in the block's scratch slab
extern "C" hipError_t smem_launch_g2a_big(const smem::G2aParams* P, uint32_t blocks, hipStream_t st);
