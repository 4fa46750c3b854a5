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
constexpr int G2A_OK = 0, G2A_UNMAPPED = 1, G2A_NOCIGAR = 2, G2A_REJECT = 3, G2A_DEFERRED = 100;
// LDS of one region in the lane-group kernels (16 / 32 / 64 lanes: 4 / 2 / 1 regions a
// wave, so 16 / 8 / 8 KB a wave) and in the scratch-tier kernel (one region per wave)
__host__ __device__ constexpr int g2a_group_lds(int group) { return group == 64 ? 8192 : 4096; }
constexpr int G2A_LDS_BIG = 32768;
// scratch-tier grid: one scratch slab per block, as many blocks as G2A_BIG_SCRATCH holds
constexpr int G2A_BIG_BLOCKS_MIN = 64, G2A_BIG_BLOCKS_MAX = 2048;
constexpr uint64_t G2A_BIG_SCRATCH = 256ull << 20;

// smem_aln_t (include/smem_gpu.h)
struct Aln {
    int64_t pos;
    int32_t is_rev, n_cigar, NM, score, tries, status;
    uint64_t cigar_off, md_off;
    int32_t md_len, pad;
};

// one region as the host prepared it (bounds checked there)
struct G2aTask {
    uint64_t q_off;     // codes[q_off .. q_off + qlen): the read's [qb, qe)
    int64_t rb, re;     // doubled coordinates, within one strand, 0 < re - rb <= G2A_MAX_TLEN
    int32_t qlen;       // qe - qb, 1 .. G2A_MAX_QLEN
    int32_t qb, l_query;
    int32_t truesc, w;  // mem_alnreg_t.truesc / .w
    uint32_t out;       // index into alns[]
};

struct G2aParams {
    const G2aTask* task;
    const uint32_t* list;  // task indices of this launch
    uint32_t n;
    const uint8_t* codes;
    const uint8_t* pac;
    int64_t l_pac;
    int8_t mat[28];
    int o_del, e_del, o_ins, e_ins, a, w;
    Aln* alns;
    uint32_t* cigar;       // pool of cigar_cap words
    char* md;              // pool of md_cap bytes
    uint64_t cigar_cap, md_cap;
    unsigned long long* cur;  // [0] cigar words claimed, [1] md bytes claimed, [2] regions deferred
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

}  // namespace smem

// regions of `P->list` on lane groups of `group` (16, 32 or 64) lanes, matrix in LDS;
// a region whose matrix does not fit is marked G2A_DEFERRED and counted in cur[2]
extern "C" hipError_t smem_launch_g2a(const smem::G2aParams* P, int group, hipStream_t st);
// one region per wave on `blocks` blocks, matrix in LDS when it fits, else in the block's scratch slab
extern "C" hipError_t smem_launch_g2a_big(const smem::G2aParams* P, uint32_t blocks, hipStream_t st);
