// Raw regions -> final regions on the device: mem_sort_and_dedup
// (software/bwamem.c:705-746), mem_test_and_remove_exact (:748-753),
// mem_mark_primary_se (:755-785) and the selection, MAPQ and flags at the head
// of mem_reg2sam_se / mem_reg2aln (:1333-1356, :1367-1379, :1498-1499, :1550).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aln_kernels.h"

namespace smem {

constexpr int FIN_LANE_MAX = 16;    // reads of up to this many raw regions: one read per lane
constexpr int FIN_MAX_REGS = 1024;  // SMEM_FIN_MAX_REGS: more raw regions reject the read
constexpr int FIN_TAB_LEN = 4096;   // SMEM_FIN_TAB_LEN: arguments the log tables cover
constexpr int FIN_REJECT = 1;       // SMEM_FIN_REJECT
// LDS of one block (one wave) of either tier: FIN_MAX_REGS regions of one read, or
// FIN_LANE_MAX regions of each of 64 reads, at 40 B a region
constexpr int FIN_LDS_BYTES = FIN_MAX_REGS * 40;
constexpr int FIN_WAVE_BLOCKS = 2048;  // the wave tier's grid (blocks take reads in turn)

// smem_fin_sel_t (include/smem_gpu.h)
struct FinSel {
    int32_t mapq, flag, xs;
};

struct FinParams {
    const AlnReg* regs;        // raw regions, reg_off[n_reads + 1]
    const uint64_t* reg_off;
    const int32_t* read_len;   // per read, or nullptr: offs[r + 1] - offs[r]
    const uint64_t* offs;
    const int64_t* ids;        // per read, or nullptr: id0 + r
    int64_t id0;
    int n_reads;
    // smem_fin_opt_t
    int a, b, o_del, e_del, o_ins, e_ins, min_seed_len, T;
    float mask_level, mask_level_redun, mapQ_coef_len;
    int mapQ_coef_fac, no_exact, all, no_multi;
    const double* log_tab;     // log(x), x in [0, FIN_TAB_LEN), from the host's libm
    const int32_t* subn_tab;   // (int)(4.343 * log(x + 1) + .499)
    // the split: [0] lane-tier reads, [1] wave-tier reads; lane_list / wave_list: n_reads each
    uint32_t* ctr;
    uint32_t* lane_list;
    uint32_t* wave_list;
    // per read: final regions, selected regions, status; the regions themselves at the
    // read's input offset until fin_write compacts them
    uint64_t* n_out;
    uint64_t* n_sel;
    int32_t* status;
    AlnReg* tmp_regs;
    FinSel* tmp_sel;
    uint32_t* tmp_idx;         // selected regions, as indices into the read's final list
    // compacted output
    const uint64_t* out_off;
    const uint64_t* sel_off;
    AlnReg* out_regs;
    FinSel* out_sel;
    uint64_t* out_idx;         // indices into out_regs
    uint64_t n_regs;
};

}  // namespace smem

// reads -> lane_list / wave_list by raw region count; rejected reads get their status here
extern "C" hipError_t smem_launch_fin_split(const smem::FinParams* P, hipStream_t st);
// the two tiers (grids sized by n_reads: the counts stay on the device)
extern "C" hipError_t smem_launch_fin_lane(const smem::FinParams* P, hipStream_t st);
extern "C" hipError_t smem_launch_fin_wave(const smem::FinParams* P, hipStream_t st);
// tmp_* -> out_* at out_off / sel_off (the scans of n_out / n_sel)
extern "C" hipError_t smem_launch_fin_write(const smem::FinParams* P, hipStream_t st);
