// Mate rescue on the device: the loop of mem_sam_pe that runs mem_matesw for
// the good hits of either end against the other end's read
// (software/bwamem_pair.c:109-175, 252-263).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fin_kernels.h"
#include "ksw_kernels.h"

namespace smem {

constexpr int MSW_HOST = 1;        // SMEM_MSW_HOST
constexpr int MSW_MAX_QLEN = 256;  // the longest mate (the SW's query columns)
constexpr int MSW_WAVES_PER_CU = 3;  // msw_wave_kernel: 49.4 KB of LDS a wave

// the fields of mem_pestat_t the rescue reads
struct MswPes {
    int32_t low, high, failed;
};

struct MswParams {
    // the pairs: reads 2p, 2p + 1 (nt4 codes) and their regions after mem_sort_and_dedup
    const uint8_t* codes;
    const uint64_t* offs;      // [2 n_pairs + 1]
    const AlnReg* regs;
    const uint64_t* reg_off;   // [2 n_pairs + 1]
    const uint8_t* pac;
    int64_t l_pac;
    int n_pairs;
    MswPes pes[4];
    int8_t mat[28];
    int o_del, e_del, o_ins, e_ins, a, min_seed_len, pen_unpaired, max_matesw;
    float mask_level_redun;
    int shift, top;            // ksw_qinit's byte bias and largest score
    // read r's two list buffers, (woff[r + 1] - woff[r]) / 2 regions each, at work + woff[r]
    AlnReg* work;
    const uint64_t* woff;      // [2 n_pairs + 1]
    uint32_t* ctr;             // [0]: pairs listed for the wave kernel
    uint32_t* wave_list;       // [n_pairs]
    uint64_t* n_out;           // [2 n_pairs] regions of each read afterwards
    uint8_t* src;              // [2 n_pairs] where they are: 0 the input list, 1 / 2 the read's work buffer
    int32_t* n_sw;             // [n_pairs]
    int32_t* status;           // [n_pairs]
    // compaction
    const uint64_t* out_off;   // [2 n_pairs + 1]
    AlnReg* out;
};

}  // namespace smem

// lane per pair: pairs left to the host, pairs no anchor of which needs an SW (both settled
// here: lists as they came, n_sw 0), the rest listed for the wave kernel
extern "C" hipError_t smem_launch_msw_pre(const smem::MswParams* P, hipStream_t st);
// wave per listed pair: the reference's loop in its order
extern "C" hipError_t smem_launch_msw_wave(const smem::MswParams* P, int n_cu, hipStream_t st);
// lists -> out at out_off (the scan of n_out), n_regs regions in all
extern "C" hipError_t smem_launch_msw_write(const smem::MswParams* P, uint64_t n_regs, hipStream_t st);
