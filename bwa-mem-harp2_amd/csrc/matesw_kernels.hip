// Mate rescue (matesw_kernels.h): lines 252-263 of software/bwamem_pair.c for
// every pair of a batch.
//
// msw_pre_kernel, a lane per pair, runs mem_matesw's skip test (:113-121) of
// every anchor against the mate's list as it came.  When no anchor gets past
// it nothing can change -- every mem_matesw call returns before it touches
// the list -- so the pair is settled: lists copied through, n = 0.
//
// msw_wave_kernel, a wave per remaining pair, walks the reference's loop in
// its order: the anchors of end 0 against end 1's list, then those of end 1
// against the list of end 0 as the first half left it.  The anchors are the
// input regions (b[0], b[1] are copied before any rescue, :255-258).  Each
// list lives in one of the read's two buffers in global scratch; an insertion
// (:160-166) and a mem_sort_and_dedup (:170) write the other buffer and swap.
// Every SW is run by the whole wave (kswd::sw_align_wave<true>), every
// mem_sort_and_dedup is fin_sort_dedup_wave over a view of the list in LDS,
// so nothing is speculated.  Everything that steers a loop is wave-uniform
// and goes through readfirstlane; a pair that meets a case left to the host
// raises a flag that ends the loops by their conditions.
//
// Compiled with -ffp-contract=off, as fin_kernels.hip is: the redundancy test
// of mem_sort_and_dedup is float arithmetic.
#include "matesw_kernels.h"
#include "fin_device.h"
#include "ksw_device.h"

namespace smem {
namespace {

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t uni64(int64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)((uint64_t)hi << 32 | lo);
}

__device__ __forceinline__ int pac_at(const uint8_t* pac, int64_t l) {
    return pac[l >> 2] >> ((~l & 3) << 1) & 3;  // _get_pac (software/bntseq.h)
}

// pes[r] by selects: a runtime index into the kernel's arguments would copy them to scratch
__device__ __forceinline__ int msw_low(const MswParams& P, int r) {
    return r == 0 ? P.pes[0].low : r == 1 ? P.pes[1].low : r == 2 ? P.pes[2].low : P.pes[3].low;
}
__device__ __forceinline__ int msw_high(const MswParams& P, int r) {
    return r == 0 ? P.pes[0].high : r == 1 ? P.pes[1].high : r == 2 ? P.pes[2].high : P.pes[3].high;
}

// bit r set: a region starting at b2 pairs with the anchor at b1 in orientation r (:117-119)
__device__ __forceinline__ int msw_found(const MswParams& P, int64_t b1, int64_t b2) {
    int64_t dist;
    const int r = pe_infer_dir(P.l_pac, b1, b2, dist);
    return dist >= (int64_t)msw_low(P, r) && dist <= (int64_t)msw_high(P, r) ? 1 << r : 0;
}

__device__ __forceinline__ int msw_failed(const MswParams& P) {
    return (P.pes[0].failed ? 1 : 0) | (P.pes[1].failed ? 2 : 0) | (P.pes[2].failed ? 4 : 0) | (P.pes[3].failed ? 8 : 0);
}

__global__ __launch_bounds__(256) void msw_pre_kernel(MswParams P) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= (uint32_t)P.n_pairs) return;
    uint64_t base[2], n[2];
    bool host = false;
    for (int e = 0; e < 2; ++e) {
        const uint64_t len = P.offs[2 * p + e + 1] - P.offs[2 * p + e];
        base[e] = P.reg_off[2 * p + e];
        n[e] = P.reg_off[2 * p + e + 1] - base[e];
        host = host || len < 1 || len > (uint64_t)MSW_MAX_QLEN || n[e] > (uint64_t)FIN_MAX_REGS;
    }
    bool need = false;
    const int failed = msw_failed(P);
    for (int i = 0; i < 2 && !host && !need; ++i) {
        if (n[i] == 0) continue;
        const AlnReg* A = P.regs + base[i];
        const AlnReg* M = P.regs + base[1 - i];
        const int floor = A[0].score - P.pen_unpaired;
        int na = 0;
        for (uint64_t j = 0; j < n[i] && na < P.max_matesw && !need; ++j) {
            if (A[j].score < floor) continue;
            ++na;
            int skip = failed;
            const int64_t b1 = A[j].rb;
            for (uint64_t k = 0; k < n[1 - i] && skip != 15; ++k) skip |= msw_found(P, b1, M[k].rb);
            need = skip != 15;
        }
    }
    for (int e = 0; e < 2; ++e) P.n_out[2 * p + e] = n[e], P.src[2 * p + e] = 0;
    P.n_sw[p] = 0;
    P.status[p] = host ? MSW_HOST : 0;
    if (need) P.wave_list[atomicAdd(&P.ctr[0], 1u)] = p;
}

__device__ __forceinline__ void msw_pair_wave(const MswParams& P, const View<1>& v, uint32_t* stk, int* blist,
                                              const int8_t* mat, uint32_t p, int lane) {
    const int64_t l_pac = P.l_pac;
    // the two ends' lists: count, buffer in use (named scalars, selected by end: arrays indexed
    // by a loop variable would live in scratch)
    const uint64_t base0 = (uint64_t)uni64((int64_t)P.reg_off[2 * p]), base1 = (uint64_t)uni64((int64_t)P.reg_off[2 * p + 1]);
    const int n_in0 = uni((int)(base1 - base0)), n_in1 = uni((int)(P.reg_off[2 * p + 2] - base1));
    const uint64_t w0 = (uint64_t)uni64((int64_t)P.woff[2 * p]), w1 = (uint64_t)uni64((int64_t)P.woff[2 * p + 1]);
    const int cap0 = uni((int)((w1 - w0) >> 1)), cap1 = uni((int)((P.woff[2 * p + 2] - w1) >> 1));
    AlnReg* const buf0 = P.work + w0;
    AlnReg* const buf1 = P.work + w1;
    int n0 = n_in0, n1 = n_in1, cur0 = 0, cur1 = 0;
    for (int k = lane; k < n_in0; k += 64) buf0[k] = P.regs[base0 + (uint64_t)k];
    for (int k = lane; k < n_in1; k += 64) buf1[k] = P.regs[base1 + (uint64_t)k];
    __syncthreads();
    const int failed = msw_failed(P);
    bool host = false;
    int n_sw = 0;
    for (int i = 0; i < 2 && !host; ++i) {
        const int m = 1 - i;
        // the mate's list (end m) for this half, written back below
        AlnReg* const bufm = m ? buf1 : buf0;
        const int capm = m ? cap1 : cap0, n_ini = i ? n_in1 : n_in0;
        int nm = m ? n1 : n0, curm = m ? cur1 : cur0;
        const uint8_t* ms = P.codes + (uint64_t)uni64((int64_t)P.offs[2 * p + m]);
        const int l_ms = uni((int)(P.offs[2 * p + m + 1] - P.offs[2 * p + m]));
        const AlnReg* A = P.regs + (i ? base1 : base0);
        const int floor = n_ini > 0 ? uni(A[0].score) - P.pen_unpaired : 0;
        int na = 0;
        for (int j = 0; j < n_ini && na < P.max_matesw && !host; ++j) {
            const bool anchor = uni(A[j].score) >= floor;   // (:257)
            if (anchor) {
                ++na;
                const int64_t arb = uni64(A[j].rb);
                // mem_matesw: orientations already found in the mate's current list (:113-120)
                const AlnReg* M = bufm + (size_t)curm * (size_t)capm;
                int mine = 0;
                for (int k0 = 0; k0 < nm; k0 += 64) {
                    const int k = k0 + lane;
                    if (k < nm) mine |= msw_found(P, arb, M[k].rb);
                }
                int skip = failed;
                for (int r = 0; r < 4; ++r)
                    if (__ballot((mine >> r) & 1)) skip |= 1 << r;
                skip = uni(skip);
                int n_loc = 0;
                for (int r = 0; r < 4 && skip != 15 && !host; ++r) {   // (:121-122)
                    if (!((skip >> r) & 1)) {
                        const bool is_rev = (r >> 1) != (r & 1), is_larger = !(r >> 1);
                        const int64_t low = msw_low(P, r), high = msw_high(P, r);
                        int64_t rb, re;
                        if (!is_rev) {                                  // (:134-140)
                            rb = is_larger ? arb + low : arb - high;
                            re = (is_larger ? arb + high : arb - low) + l_ms;
                        } else {
                            rb = (is_larger ? arb + low : arb - high) - l_ms;
                            re = is_larger ? arb + high : arb - low;
                        }
                        if (rb < 0) rb = 0;
                        if (re > l_pac << 1) re = l_pac << 1;
                        // bns_get_seq (software/bntseq.c:355-376) returns re - rb bases unless the
                        // ends are out of order or the window bridges l_pac (:144)
                        const bool run = re >= rb && (rb >= l_pac || re <= l_pac);
                        if (run && re - rb > (int64_t)KSWA_MAX_TLEN) host = true;
                        if (run && !host) {
                            const int len = (int)(re - rb);
                            const int xtra = kswd::SW_XSUBO | kswd::SW_XSTART | (l_ms * P.a < 250 ? kswd::SW_XBYTE : 0) |
                                             (P.min_seed_len * P.a);   // (:147)
                            const kswd::SwAlign aln = kswd::sw_align_wave<true>(
                                l_ms,
                                [&](int q) {
                                    if (!is_rev) return (int)ms[q];
                                    const int c = ms[l_ms - 1 - q];
                                    return c < 4 ? 3 - c : 4;
                                },
                                len,
                                [&](int t) {
                                    const int64_t x = rb + t;
                                    return x < l_pac ? pac_at(P.pac, x) : 3 - pac_at(P.pac, (l_pac << 1) - 1 - x);
                                },
                                mat, P.o_del, P.e_del, P.o_ins, P.e_ins, xtra, P.shift, P.top, blist);
                            const int score = uni(aln.score), qb = uni(aln.qb);
                            if (score >= P.min_seed_len && qb >= 0) {   // (:150)
                                if (nm + 1 > FIN_MAX_REGS || nm + 1 > capm) {
                                    host = true;
                                } else {
                                    const int qe = uni(aln.qe), tb = uni(aln.tb), te = uni(aln.te);
                                    // before the first lower score (:160-166), into the other buffer
                                    const AlnReg* S = bufm + (size_t)curm * (size_t)capm;
                                    AlnReg* D = bufm + (size_t)(curm ^ 1) * (size_t)capm;
                                    int at = nm;
                                    for (int k0 = 0; k0 < nm; k0 += 64) {
                                        const int k = k0 + lane;
                                        if (k < nm && S[k].score < score && k < at) at = k;
                                    }
                                    at = uni(-kswd::wave_max(-at));
                                    for (int k0 = 0; k0 <= nm; k0 += 64) {
                                        const int k = k0 + lane;
                                        if (k <= nm && k != at) D[k] = S[k < at ? k : k - 1];
                                    }
                                    if (lane == 0) {
                                        AlnReg* const B = D + at;
                                        B->qb = is_rev ? l_ms - (qe + 1) : qb;    // (:151-158)
                                        B->qe = is_rev ? l_ms - qb : qe + 1;
                                        B->rb = is_rev ? (l_pac << 1) - (rb + te + 1) : rb + tb;
                                        B->re = is_rev ? (l_pac << 1) - (rb + tb) : rb + te + 1;
                                        B->score = score, B->truesc = 0, B->sub = 0, B->csub = uni(aln.score2);
                                        B->sub_n = 0, B->w = 0, B->secondary = -1, B->hash = 0;
                                        const int64_t rl_ = B->re - B->rb;
                                        const int ql_ = B->qe - B->qb;
                                        B->seedcov = (int)((rl_ < (int64_t)ql_ ? rl_ : (int64_t)ql_) >> 1);
                                    }
                                    curm ^= 1;
                                    ++nm;
                                    __syncthreads();
                                }
                            }
                            if (!host) ++n_loc;   // (:168)
                        }
                        if (!host && n_loc > 0 && nm > 1) {   // mem_sort_and_dedup (:170)
                            const AlnReg* S = bufm + (size_t)curm * (size_t)capm;
                            AlnReg* D = bufm + (size_t)(curm ^ 1) * (size_t)capm;
                            for (int k = lane; k < nm; k += 64) {
                                const AlnReg& R = S[k];
                                v.KA(k) = R.re, v.KB(k) = R.rb, v.QB(k) = R.qb, v.QE(k) = R.qe, v.SC(k) = R.score;
                                v.P(k) = (uint32_t)k;
                            }
                            __syncthreads();
                            const int kept = uni((int)fin_sort_dedup_wave(v, (uint32_t)nm, P.mask_level_redun, stk, lane));
                            __syncthreads();
                            for (int k = lane; k < kept; k += 64) D[k] = S[v.P((uint32_t)k)];
                            curm ^= 1;
                            nm = kept;
                            __syncthreads();
                        }
                    }
                }
                n_sw += n_loc;
            }
        }
        if (m) n1 = nm, cur1 = curm;
        else n0 = nm, cur0 = curm;
    }
    if (lane == 0) {
        if (host) {
            P.status[p] = MSW_HOST;   // the lists as they came and n_sw = 0 are msw_pre_kernel's
        } else {
            P.n_out[2 * p] = (uint64_t)n0, P.src[2 * p] = (uint8_t)(1 + cur0);
            P.n_out[2 * p + 1] = (uint64_t)n1, P.src[2 * p + 1] = (uint8_t)(1 + cur1);
            P.n_sw[p] = n_sw;
        }
    }
}

__global__ __launch_bounds__(64) void msw_wave_kernel(MswParams P) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[FIN_LDS_BYTES];
    __shared__ uint32_t stk[3 * FIN_STK];
    __shared__ int blist[2 * KSWA_B_MAX];
    // the scoring matrix in LDS: the SW indexes it by query code, and a runtime index into the
    // kernel's arguments would put a copy of them in scratch
    __shared__ int8_t mat[32];
#pragma unroll
    for (int k = 0; k < 25; ++k)
        if (threadIdx.x == 0) mat[k] = P.mat[k];
    __syncthreads();
    const uint32_t n = P.ctr[0];
    for (uint32_t w = blockIdx.x; w < n; w += gridDim.x) {
        msw_pair_wave(P, make_view<1>(lds, 0), stk, blist, mat, P.wave_list[w], (int)threadIdx.x);
        __syncthreads();
    }
}

// one thread per output region
__global__ __launch_bounds__(256) void msw_write_kernel(MswParams P, uint64_t n_regs) {
    const uint64_t o = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (o >= n_regs) return;
    uint32_t lo = 0, hi = 2u * (uint32_t)P.n_pairs;  // the last r with out_off[r] <= o
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (P.out_off[mid] <= o) lo = mid;
        else hi = mid;
    }
    const uint32_t r = lo;
    const uint64_t k = o - P.out_off[r];
    if (k >= P.n_out[r]) return;
    const uint32_t s = P.src[r];
    const AlnReg* from = s == 0 ? P.regs + P.reg_off[r]
                                : P.work + P.woff[r] + (uint64_t)(s - 1) * ((P.woff[r + 1] - P.woff[r]) >> 1);
    P.out[o] = from[k];
}

}  // namespace
}  // namespace smem

extern "C" hipError_t smem_launch_msw_pre(const smem::MswParams* P, hipStream_t st) {
    if (P->n_pairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(smem::msw_pre_kernel, dim3((unsigned)((P->n_pairs + 255) / 256)), dim3(256), 0, st, *P);
    return hipGetLastError();
}

extern "C" hipError_t smem_launch_msw_wave(const smem::MswParams* P, int n_cu, hipStream_t st) {
    if (P->n_pairs <= 0) return hipSuccess;
    const int slots = n_cu * smem::MSW_WAVES_PER_CU;
    hipLaunchKernelGGL(smem::msw_wave_kernel, dim3((unsigned)(P->n_pairs < slots ? P->n_pairs : slots)), dim3(64), 0, st,
                       *P);
    return hipGetLastError();
}

extern "C" hipError_t smem_launch_msw_write(const smem::MswParams* P, uint64_t n_regs, hipStream_t st) {
    if (n_regs == 0) return hipSuccess;
    hipLaunchKernelGGL(smem::msw_write_kernel, dim3((unsigned)((n_regs + 255) / 256)), dim3(256), 0, st, *P, n_regs);
    return hipGetLastError();
}
