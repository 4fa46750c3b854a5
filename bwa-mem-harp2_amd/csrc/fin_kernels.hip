// Raw regions -> final regions (fin_kernels.h).  Two tiers by a read's raw
// region count: up to FIN_LANE_MAX, one read per lane, everything serial as
// the reference wrote it; above, one read per wave -- the three sorts run on
// lane 0 (ks_introsort is not stable for n >= 3, software/ksort.h:176-226, so
// they are emulated comparison for comparison on a permutation in LDS; the
// records never move), the inner loops of the de-duplication and of
// mem_mark_primary_se are ballots over 64 candidates, the compactions are
// prefix ranks, and selection, MAPQ and flags are one region per lane.
//
// Arithmetic that decides parity: the two overlap tests are float products
// (software/bwamem.c:721, 774), MAPQ is double arithmetic truncated to int
// (:1340-1352).  This file is compiled with -ffp-contract=off and the
// functions below say so again: a fused multiply-add would round once where
// the host rounds twice.  log() comes from tables the host filled with its own
// libm; the division by log(l) is an IEEE division on both sides (fin_mapq, in
// fin_device.h: the pairing stage calls it too).
#include "fin_kernels.h"
#include "fin_device.h"

namespace smem {
namespace {

// the third order (software/bwamem.c:696-703), over regions
template <int S>
struct LtHash {
    View<S> v;
    __device__ __forceinline__ bool operator()(uint32_t x, uint32_t y) const {
        const int sx = v.SC(x), sy = v.SC(y);
        return sx > sy || (sx == sy && (uint64_t)v.KA(x) < (uint64_t)v.KA(y));
    }
};

// "significant overlap" on the query (software/bwamem.c:770-774)
__device__ __forceinline__ bool fin_overlaps(float ml, int jqb, int jqe, int iqb, int iqe) {
#pragma clang fp contract(off)
    const int b_max = jqb > iqb ? jqb : iqb;
    const int e_min = jqe < iqe ? jqe : iqe;
    if (e_min <= b_max) return false;
    const int min_l = iqe - iqb < jqe - jqb ? iqe - iqb : jqe - jqb;
    return (float)(e_min - b_max) >= (float)min_l * ml;
}

struct ReadArgs {
    uint64_t base;   // the read's first raw region
    uint32_t n;      // raw regions
    int64_t id;
    int qlen;
};

__device__ __forceinline__ ReadArgs fin_read_args(const FinParams& P, uint32_t r) {
    ReadArgs A;
    A.base = P.reg_off[r];
    A.n = (uint32_t)(P.reg_off[r + 1] - A.base);
    A.id = P.ids ? P.ids[r] : P.id0 + (int64_t)r;
    A.qlen = P.read_len ? P.read_len[r] : (int)(P.offs[r + 1] - P.offs[r]);
    return A;
}

// the record and the selection of the region at final position k (software/bwamem.c:1370-1378,
// 1498-1499, 1550); returns the flag (-1: no record), mapq before the cap
template <int S>
__device__ __forceinline__ int fin_emit(const FinParams& P, const View<S>& v, const ReadArgs& A, uint32_t k,
                                        int& mapq, int& xs) {
    const uint32_t x = v.P(k);
    AlnReg R = P.regs[A.base + x];
    const uint32_t aux = v.AUX(x);
    const int sec = (int)(aux & 0xffffu) - 1;
    R.sub = v.SUB(x);
    R.sub_n += (int32_t)(aux >> 16);
    R.secondary = sec;
    R.hash = (uint64_t)v.KA(x);
    P.tmp_regs[A.base + k] = R;
    mapq = 0, xs = 0;
    if (R.score < P.T) return -1;
    if (sec >= 0 && !P.all) return -1;
    if (sec >= 0 && (double)R.score < (double)v.SC(v.P((uint32_t)sec)) * .5) return -1;
    if (sec >= 0) {
        xs = -1;
        return 0x100;
    }
    const int l = R.qe - R.qb > v.RLEN(x) ? R.qe - R.qb : v.RLEN(x);
    mapq = fin_mapq(P, R.score, R.sub, R.csub, l, R.seedcov, R.sub_n);
    xs = R.sub > R.csub ? R.sub : R.csub;
    return k ? (P.no_multi ? 0x10000 : 0x800) : 0;
}

// ------------------------------------------------------------- lane tier
// (SMALL / S are parameters so that the same text also runs one big read serially: the
// kernels instantiate <true, 64> only)
template <bool SMALL, int S>
__device__ void fin_read_lane(const FinParams& P, const View<S>& v0, uint32_t* stk, uint32_t r) {
    View<S> v = v0;
    const ReadArgs A = fin_read_args(P, r);
    uint32_t n = A.n;
    for (uint32_t k = 0; k < n; ++k) {
        const AlnReg& R = P.regs[A.base + k];
        v.KA(k) = R.re, v.KB(k) = R.rb, v.QB(k) = R.qb, v.QE(k) = R.qe, v.SC(k) = R.score;
        v.SUB(k) = 0, v.AUX(k) = 0, v.P(k) = k;
    }
    if (n > 1) {  // mem_sort_and_dedup
        fin_introsort<SMALL>(v, n, LtRe<S>{v}, stk);
        for (uint32_t i = 1; i < n; ++i) {
            const uint32_t p = v.P(i);
            const int64_t prb = v.KB(p), pre = v.KA(p);
            if (prb >= v.KA(v.P(i - 1))) continue;
            const int pqb = v.QB(p), pqe = v.QE(p), psc = v.SC(p);
            for (int j = (int)i - 1; j >= 0; --j) {
                const uint32_t q = v.P((uint32_t)j);
                const int64_t qre = v.KA(q);
                if (!(prb < qre)) break;
                const int qqb = v.QB(q), qqe = v.QE(q);
                if (qqe == qqb) continue;
                if (fin_redundant(P.mask_level_redun, prb, pre, pqb, pqe, v.KB(q), qre, qqb, qqe)) {
                    if (psc < v.SC(q)) {
                        v.QE(p) = pqb;
                        break;
                    }
                    v.QE(q) = qqb;
                }
            }
        }
        uint32_t m = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t x = v.P(i);
            if (v.QE(x) > v.QB(x)) v.P(m++) = x;
        }
        if (m == 0) {
            n = 1;  // the reference's second pass starts its count at 1 (software/bwamem.c:740)
        } else {
            n = m;
            fin_introsort<SMALL>(v, n, LtScore<S>{v}, stk);
            // "mark identical hits" compares fields the marking does not touch
            m = 1;
            uint32_t prev = v.P(0);
            for (uint32_t i = 1; i < n; ++i) {
                const uint32_t x = v.P(i);
                const bool same = v.SC(x) == v.SC(prev) && v.KB(x) == v.KB(prev) && v.QB(x) == v.QB(prev);
                prev = x;
                if (!same) v.P(m++) = x;
            }
            n = m;
        }
    }
    // mem_test_and_remove_exact
    if (P.no_exact && n > 0 && P.regs[A.base + v.P(0)].truesc == A.qlen * P.a) v.perm += S, --n;
    uint32_t n_sel = 0;
    if (n > 0) {  // mem_mark_primary_se
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t x = v.P(k);
            const int rlen = (int)(v.KA(x) - v.KB(x));
            v.KA(x) = (int64_t)fin_hash_64((uint64_t)(A.id + (int64_t)k));
            v.RLEN(x) = rlen;
        }
        fin_introsort<SMALL>(v, n, LtHash<S>{v}, stk);
        int tmp = P.a + P.b;
        tmp = P.o_del + P.e_del > tmp ? P.o_del + P.e_del : tmp;
        tmp = P.o_ins + P.e_ins > tmp ? P.o_ins + P.e_ins : tmp;
        for (uint32_t i = 1; i < n; ++i) {
            const uint32_t p = v.P(i);
            const int pqb = v.QB(p), pqe = v.QE(p), psc = v.SC(p);
            for (uint32_t j = 0; j < i; ++j) {
                const uint32_t q = v.P(j);
                if (v.AUX(q) & 0xffffu) continue;  // not in z
                if (fin_overlaps(P.mask_level, v.QB(q), v.QE(q), pqb, pqe)) {
                    if (v.SUB(q) == 0) v.SUB(q) = psc;
                    if (v.SC(q) - psc <= tmp) v.AUX(q) += 1u << 16;
                    v.AUX(p) |= j + 1;
                    break;
                }
            }
        }
        int first = 0;
        for (uint32_t k = 0; k < n; ++k) {
            int mapq, xs;
            const int flag = fin_emit(P, v, A, k, mapq, xs);
            if (flag >= 0) {
                if (n_sel == 0) first = mapq;
                else if (mapq > first) mapq = first;
                P.tmp_idx[A.base + n_sel++] = k;
            }
            P.tmp_sel[A.base + k] = FinSel{mapq, flag, xs};
        }
    }
    P.n_out[r] = n, P.n_sel[r] = n_sel, P.status[r] = 0;
}

__global__ __launch_bounds__(64) void fin_lane_kernel(FinParams P) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[FIN_LDS_BYTES];
    const uint32_t t = blockIdx.x * 64u + threadIdx.x;
    if (t >= P.ctr[0]) return;
    fin_read_lane<true, 64>(P, make_view<64>(lds, (int)threadIdx.x), nullptr, P.lane_list[t]);
}

// ------------------------------------------------------------- wave tier
__device__ void fin_read_wave(const FinParams& P, const View<1>& v0, uint32_t* stk, uint32_t r, int lane) {
    View<1> v = v0;
    const ReadArgs A = fin_read_args(P, r);
    uint32_t n = A.n;
    for (uint32_t k = (uint32_t)lane; k < n; k += 64) {
        const AlnReg& R = P.regs[A.base + k];
        v.KA(k) = R.re, v.KB(k) = R.rb, v.QB(k) = R.qb, v.QE(k) = R.qe, v.SC(k) = R.score;
        v.SUB(k) = 0, v.AUX(k) = 0, v.P(k) = k;
    }
    __syncthreads();
    if (n > 1) n = fin_sort_dedup_wave(v, n, P.mask_level_redun, stk, lane);  // mem_sort_and_dedup
    // mem_test_and_remove_exact
    if (P.no_exact && n > 0 && P.regs[A.base + v.P(0)].truesc == A.qlen * P.a) v.perm += 1, --n;
    uint32_t n_sel = 0;
    if (n > 0) {  // mem_mark_primary_se
        for (uint32_t k = (uint32_t)lane; k < n; k += 64) {
            const uint32_t x = v.P(k);
            const int rlen = (int)(v.KA(x) - v.KB(x));
            v.KA(x) = (int64_t)fin_hash_64((uint64_t)(A.id + (int64_t)k));
            v.RLEN(x) = rlen;
        }
        __syncthreads();
        if (lane == 0) fin_introsort<false>(v, n, LtHash<1>{v}, stk);
        __syncthreads();
        int tmp = P.a + P.b;
        tmp = P.o_del + P.e_del > tmp ? P.o_del + P.e_del : tmp;
        tmp = P.o_ins + P.e_ins > tmp ? P.o_ins + P.e_ins : tmp;
        for (uint32_t i = 1; i < n; ++i) {
            const uint32_t p = v.P(i);
            const int pqb = v.QB(p), pqe = v.QE(p), psc = v.SC(p);
            // the first z entry with a significant overlap: z is the positions below i
            // that are not secondary, in order
            for (uint32_t b = 0; b < i; b += 64) {
                const uint32_t j = b + (uint32_t)lane;
                uint32_t q = 0;
                bool hit = false;
                if (j < i) {
                    q = v.P(j);
                    hit = !(v.AUX(q) & 0xffffu) && fin_overlaps(P.mask_level, v.QB(q), v.QE(q), pqb, pqe);
                }
                const uint64_t m_hit = __ballot(hit);
                if (m_hit) {
                    if (lane == __builtin_ctzll(m_hit)) {
                        if (v.SUB(q) == 0) v.SUB(q) = psc;
                        if (v.SC(q) - psc <= tmp) v.AUX(q) += 1u << 16;
                        v.AUX(p) |= j + 1;
                    }
                    break;
                }
            }
            __syncthreads();
        }
        int first = 0;
        const uint64_t below = (1ull << lane) - 1;
        for (uint32_t b = 0; b < n; b += 64) {
            const uint32_t k = b + (uint32_t)lane;
            int mapq = 0, xs = 0, flag = -1;
            if (k < n) flag = fin_emit(P, v, A, k, mapq, xs);
            const uint64_t m_sel = __ballot(flag >= 0);
            if (m_sel) {
                const int l0 = __builtin_ctzll(m_sel);
                const int got = __shfl(mapq, l0);
                if (n_sel == 0) {
                    first = got;
                    if (flag >= 0 && lane != l0 && mapq > first) mapq = first;
                } else if (flag >= 0 && mapq > first) {
                    mapq = first;
                }
                if (flag >= 0) P.tmp_idx[A.base + n_sel + (uint32_t)__builtin_popcountll(m_sel & below)] = k;
                n_sel += (uint32_t)__builtin_popcountll(m_sel);
            }
            if (k < n) P.tmp_sel[A.base + k] = FinSel{mapq, flag, xs};
        }
    }
    if (lane == 0) P.n_out[r] = n, P.n_sel[r] = n_sel, P.status[r] = 0;
}

__global__ __launch_bounds__(64) void fin_wave_kernel(FinParams P) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[FIN_LDS_BYTES];
    __shared__ uint32_t stk[3 * FIN_STK];
    const uint32_t n = P.ctr[1];
    for (uint32_t w = blockIdx.x; w < n; w += gridDim.x) {
        fin_read_wave(P, make_view<1>(lds, 0), stk, P.wave_list[w], (int)threadIdx.x);
        __syncthreads();
    }
}

// ------------------------------------------------------------- split / write
__global__ __launch_bounds__(256) void fin_split_kernel(FinParams P) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= (uint32_t)P.n_reads) return;
    const uint64_t n = P.reg_off[r + 1] - P.reg_off[r];
    if (n > (uint64_t)FIN_MAX_REGS) {
        P.n_out[r] = 0, P.n_sel[r] = 0, P.status[r] = FIN_REJECT;
    } else if (n <= (uint64_t)FIN_LANE_MAX) {
        P.lane_list[atomicAdd(&P.ctr[0], 1u)] = r;
    } else {
        P.wave_list[atomicAdd(&P.ctr[1], 1u)] = r;
    }
}

// one thread per raw region slot i: slot k = i - reg_off[r] of its read r
__global__ __launch_bounds__(256) void fin_write_kernel(FinParams P) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= P.n_regs) return;
    uint32_t lo = 0, hi = (uint32_t)P.n_reads;  // the last r with reg_off[r] <= i
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (P.reg_off[mid] <= i) lo = mid;
        else hi = mid;
    }
    const uint32_t r = lo;
    const uint64_t k = i - P.reg_off[r];
    if (k < P.n_out[r]) {
        const uint64_t o = P.out_off[r] + k;
        P.out_regs[o] = P.tmp_regs[i];
        P.out_sel[o] = P.tmp_sel[i];
    }
    if (k < P.n_sel[r]) P.out_idx[P.sel_off[r] + k] = P.out_off[r] + P.tmp_idx[i];
}

}  // namespace
}  // namespace smem

extern "C" hipError_t smem_launch_fin_split(const smem::FinParams* P, hipStream_t st) {
    if (P->n_reads <= 0) return hipSuccess;
    hipLaunchKernelGGL(smem::fin_split_kernel, dim3((unsigned)((P->n_reads + 255) / 256)), dim3(256), 0, st, *P);
    return hipGetLastError();
}

extern "C" hipError_t smem_launch_fin_lane(const smem::FinParams* P, hipStream_t st) {
    if (P->n_reads <= 0) return hipSuccess;
    hipLaunchKernelGGL(smem::fin_lane_kernel, dim3((unsigned)((P->n_reads + 63) / 64)), dim3(64), 0, st, *P);
    return hipGetLastError();
}

extern "C" hipError_t smem_launch_fin_wave(const smem::FinParams* P, hipStream_t st) {
    if (P->n_reads <= 0) return hipSuccess;
    const unsigned grid = (unsigned)(P->n_reads < smem::FIN_WAVE_BLOCKS ? P->n_reads : smem::FIN_WAVE_BLOCKS);
    hipLaunchKernelGGL(smem::fin_wave_kernel, dim3(grid), dim3(64), 0, st, *P);
    return hipGetLastError();
}

extern "C" hipError_t smem_launch_fin_write(const smem::FinParams* P, hipStream_t st) {
    if (P->n_regs == 0) return hipSuccess;
    hipLaunchKernelGGL(smem::fin_write_kernel, dim3((unsigned)((P->n_regs + 255) / 256)), dim3(256), 0, st, *P);
    return hipGetLastError();
}
