// The two steps of mem_sam_pe around mate rescue, on the device: the per-pair part of
// mem_pestat (software/bwamem_pair.c:52-63; the finish over the histogram is the host's) and
// mem_pair with the decision block around it (:177-236, :264-304, :321-326).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fin_kernels.h"

namespace smem {

constexpr int PST_MAX_INS = 65535;     // SMEM_PESTAT_MAX_INS
constexpr int PST_WAVES_PER_CU = 8;    // pst_kernel: blocks of 256, grid-stride over pairs
constexpr int PAIR_HOST = 1;           // SMEM_PAIR_HOST
constexpr int PAIR_TAB_LEN = 65536;    // SMEM_PAIR_TAB_LEN
constexpr int PAIR_LANE_MAX = 16;      // pairs of up to this many regions in both lists: one pair per lane
constexpr int PAIR_MAX_KEYS = 2 * FIN_MAX_REGS;
constexpr int PAIR_LDS_BYTES = PAIR_MAX_KEYS * 16;   // one long pair's keys, or PAIR_LANE_MAX keys of 64 pairs
constexpr int PAIR_WAVES_PER_CU = 4;   // pair_wave_kernel: 32 KB of LDS a wave

struct PstParams {
    const AlnReg* regs;        // each read's list after mem_sort_and_dedup
    const uint64_t* reg_off;   // [2 n_pairs + 1]
    int64_t l_pac;
    int n_pairs;
    int a, min_seed_len, max_ins;
    float mask_level;
    uint32_t* hist;            // [4][max_ins + 1]
};

// smem_pair_sel_t (include/smem_gpu.h)
struct PairSel {
    int32_t status, branch, z[2], mapq[2], proper, o, subo, n_sub, sub[2], promoted[2];
};

// one orientation: mem_pestat_t's bounds and where its row of the penalty table starts
struct PairDir {
    int32_t low, high, failed, pad;
    uint64_t tab_off;
};

struct PairParams {
    const AlnReg* regs;        // each read's list after mem_mark_primary_se
    const uint64_t* reg_off;   // [2 n_pairs + 1]
    const int64_t* ids;        // per pair, or nullptr: id0 + p
    int64_t id0;
    int64_t l_pac;
    int n_pairs;
    // smem_pair_opt_t (the names fin_mapq reads are FinParams')
    int a, b, o_del, e_del, o_ins, e_ins, pen_unpaired, T, min_seed_len, mapQ_coef_fac, nopairing;
    float mapQ_coef_len;
    const double* log_tab;     // the finalize stage's tables
    const int32_t* subn_tab;
    const PairDir* dirs;       // [4]
    const double* pen;         // .721 * log(2 erfc(|ns| / sqrt 2)) * a per orientation and distance, the host's libm
    uint32_t* ctr;             // [0] lane-tier pairs, [1] wave-tier pairs
    uint32_t* lane_list;       // [n_pairs]
    uint32_t* wave_list;       // [n_pairs]
    PairSel* sel;              // [n_pairs]
};

}  // namespace smem

// lane per pair, grid-stride: cal_sub of both ends, the uniqueness tests, mem_infer_dir, one
// count into hist[dir][is]
extern "C" hipError_t smem_launch_pst(const smem::PstParams* P, int n_cu, hipStream_t st);
// pairs -> lane_list / wave_list by the regions of both ends; pairs left to the host settled here
extern "C" hipError_t smem_launch_pair_split(const smem::PairParams* P, hipStream_t st);
extern "C" hipError_t smem_launch_pair_lane(const smem::PairParams* P, hipStream_t st);
extern "C" hipError_t smem_launch_pair_wave(const smem::PairParams* P, int n_cu, hipStream_t st);
