// Insert-size statistics and pairing (pair_kernels.h): the steps of mem_sam_pe on either
// side of mate rescue.
//
// pst_kernel, a lane per pair and grid-stride over the pairs, is lines 52-63 of
// software/bwamem_pair.c: cal_sub of both ends (a sequential scan that stops at the first
// significant overlap, over lists of any length), the two uniqueness tests, mem_infer_dir of the
// two first regions and one count into hist[dir][is].  The histogram is all that crosses to the
// host, which runs lines 64-106 over it in ascending order.
//
// The pairing kernels are mem_pair (:177-236) and the decision block (:266-304, :321-326), a
// pair per lane (pair_lane_kernel, up to PAIR_LANE_MAX regions in both lists) or per wave
// (pair_wave_kernel, up to FIN_MAX_REGS regions an end), the 128-bit keys in LDS.  pair64_lt is
// a total order on the keys, which are distinct, so any sort gives the reference's v: an
// insertion sort in the lane tier, a bitonic network in the wave tier.  The array u is never
// built.  One pass over the walk-back scan keeps the largest (q << 32 | hash, k << 32 | i), the
// largest q among the others (u[n - 2]'s) and the count; a second pass counts the candidates
// with sub - q <= tmp, of which the best is always one.  In the wave tier lane l scans the
// positions i = l, l + 64, ..: y[which] at position i is the last position below i of that
// class, and the scan skips every other class, so a walk from i - 1 meets what the reference's
// walk from y[which] meets.
//
// Arithmetic that decides parity: cal_sub's overlap test is a float product; a candidate's score
// is two double additions to a table entry the host computed with its own libm (no log, erfc or
// multiplication here), truncated after an explicit test for a sum that is not finite or is
// negative.  Compiled with -ffp-contract=off, as fin_kernels.hip is.
#include "pair_kernels.h"
#include "fin_device.h"

namespace smem {
namespace {

// ------------------------------------------------------------- mem_pestat, per pair
// cal_sub (software/bwamem_pair.c:32-44)
__device__ __forceinline__ int pst_cal_sub(const PstParams& P, const AlnReg* A, uint64_t n) {
#pragma clang fp contract(off)
    const int qb0 = A[0].qb, qe0 = A[0].qe;
    for (uint64_t j = 1; j < n; ++j) {
        const int qb = A[j].qb, qe = A[j].qe;
        const int b_max = qb > qb0 ? qb : qb0;
        const int e_min = qe < qe0 ? qe : qe0;
        if (e_min > b_max) {
            const int min_l = qe - qb < qe0 - qb0 ? qe - qb : qe0 - qb0;
            if ((float)(e_min - b_max) >= (float)min_l * P.mask_level) return A[j].score;
        }
    }
    return P.min_seed_len * P.a;
}

__global__ __launch_bounds__(256) void pst_kernel(PstParams P) {
    const uint32_t stride = gridDim.x * 256u;
    const uint32_t row = (uint32_t)P.max_ins + 1u;
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < (uint32_t)P.n_pairs; p += stride) {
        const uint64_t b0 = P.reg_off[2 * p], b1 = P.reg_off[2 * p + 1], e1 = P.reg_off[2 * p + 2];
        if (b1 == b0 || e1 == b1) continue;                                              // (:58)
        const AlnReg* A0 = P.regs + b0;
        const AlnReg* A1 = P.regs + b1;
        if ((double)pst_cal_sub(P, A0, b1 - b0) > 0.8 * (double)A0[0].score) continue;   // (:59)
        if ((double)pst_cal_sub(P, A1, e1 - b1) > 0.8 * (double)A1[0].score) continue;   // (:60)
        int64_t is;
        const int dir = pe_infer_dir(P.l_pac, A0[0].rb, A1[0].rb, is);
        if (is != 0 && is <= (int64_t)P.max_ins) atomicAdd(&P.hist[(uint32_t)dir * row + (uint32_t)is], 1u);   // (:62)
    }
}

// ------------------------------------------------------------- mem_pair
// the sorted keys of one pair in LDS, element i at [i * S] (S as in fin_device.h's View)
template <int S>
struct Keys {
    uint64_t* x;   // forward position
    uint64_t* y;   // score << 32 | i << 2 | strand << 1 | end
    __device__ __forceinline__ uint64_t& X(int i) const { return x[i * S]; }
    __device__ __forceinline__ uint64_t& Y(int i) const { return y[i * S]; }
};

__device__ __forceinline__ void pair_key(const AlnReg& R, int64_t l_pac, int i, int end, uint64_t& x, uint64_t& y) {   // (:186-187)
    x = (uint64_t)(R.rb < l_pac ? R.rb : (l_pac << 1) - 1 - R.rb);
    y = (uint64_t)(int64_t)R.score << 32 | (uint64_t)(uint32_t)(i << 2 | (R.rb >= l_pac ? 2 : 0) | end);
}

// what the stage keeps of u: its largest entry, the largest q among the others (u[n - 2].x >> 32), its size
struct Acc {
    uint64_t bx, by;
    int sub;
    uint32_t n;
};

__device__ __forceinline__ bool pair_gt(uint64_t ax, uint64_t ay, uint64_t bx, uint64_t by) {
    return ax > bx || (ax == bx && ay > by);
}

__device__ __forceinline__ void acc_add(Acc& A, uint64_t x, uint64_t y) {
    const int q = (int)(x >> 32);
    if (A.n == 0) {
        A.bx = x, A.by = y;
    } else if (pair_gt(x, y, A.bx, A.by)) {
        A.sub = (int)(A.bx >> 32);   // the former best has the largest q of all that came before
        A.bx = x, A.by = y;
    } else if (q > A.sub) {
        A.sub = q;
    }
    ++A.n;
}

__device__ __forceinline__ void acc_merge(Acc& A, const Acc& B) {
    if (B.n == 0) return;
    if (A.n == 0) {
        A = B;
        return;
    }
    int sub = A.sub > B.sub ? A.sub : B.sub;
    if (pair_gt(B.bx, B.by, A.bx, A.by)) {
        const int q = (int)(A.bx >> 32);
        sub = q > sub ? q : sub;
        A.bx = B.bx, A.by = B.by;
    } else {
        const int q = (int)(B.bx >> 32);
        sub = q > sub ? q : sub;
    }
    A.sub = sub;
    A.n += B.n;
}

// the walk-back scan of position i (:195-218).  COUNT: the candidates with sub - q <= tmp
// instead of the accumulator.
template <int S, bool COUNT>
__device__ __forceinline__ void pair_scan(const PairParams& P, const Keys<S>& K, int i, uint64_t idx, int sub, int tmp,
                                          Acc& A, uint32_t& cnt) {
#pragma clang fp contract(off)
    const uint64_t xi = K.X(i), yi = K.Y(i);
    for (int r = 0; r < 2; ++r) {
        const int dir = r << 1 | (int)(yi >> 1 & 1);
        const PairDir D = P.dirs[dir];
        if (D.failed) continue;
        const uint32_t which = (uint32_t)(r << 1) | (((uint32_t)yi & 1u) ^ 1u);
        const double* pen = P.pen + D.tab_off;
        for (int k = i - 1; k >= 0; --k) {
            const uint64_t yk = K.Y(k);
            if (((uint32_t)yk & 3u) != which) continue;
            const int64_t dist = (int64_t)(xi - K.X(k));
            if (dist > (int64_t)D.high) break;
            if (dist < (int64_t)D.low) continue;
            double s = (double)((yi >> 32) + (yk >> 32));
            s = s + pen[dist - (int64_t)D.low];
            s = s + .499;
            // a sum that is not finite, negative, or past an int: INT_MIN on the host, then the clamp (:211-212)
            const int q = s >= 0. && s < 2147483648. ? (int)s : 0;
            if (COUNT) {
                if (sub - q <= tmp) ++cnt;
            } else {
                const uint64_t py = (uint64_t)(uint32_t)k << 32 | (uint32_t)i;
                acc_add(A, (uint64_t)(uint32_t)q << 32 | (fin_hash_64(py ^ idx) & 0xffffffffull), py);
            }
        }
    }
}

__device__ __forceinline__ int pair_tmp(const PairParams& P) {   // (:222-224)
    int tmp = P.a + P.b;
    tmp = tmp > P.o_del + P.e_del ? tmp : P.o_del + P.e_del;
    tmp = tmp > P.o_ins + P.e_ins ? tmp : P.o_ins + P.e_ins;
    return tmp;
}

// id << 8 of an int: the shift in 32 bits, sign-extended for the XOR (:215)
__device__ __forceinline__ uint64_t pair_id_bits(const PairParams& P, uint32_t p) {
    const int64_t id = P.ids ? P.ids[p] : P.id0 + (int64_t)p;
    return (uint64_t)(int64_t)(int32_t)((uint32_t)id << 8);
}

__device__ __forceinline__ int pair_raw_mapq(int diff, int a) {   // raw_mapq (:238)
#pragma clang fp contract(off)
    double x = 6.02 * (double)diff;
    x = x / (double)a;
    x = x + .499;
    return (int)x;
}

// lines 291-299 for the chosen region z of one end: its MAPQ, or -1 where fin_mapq's tables end
__device__ __forceinline__ int pair_end_mapq(const PairParams& P, const AlnReg* L, int z, int q_pe, int& sub, int& promoted) {
    const AlnReg C = L[z];
    sub = C.sub, promoted = 0;
    if (C.secondary >= 0) sub = L[C.secondary].score, promoted = 1;   // (:290-291)
    const int64_t rl = C.re - C.rb;
    const int l = (int64_t)(C.qe - C.qb) > rl ? C.qe - C.qb : (int)rl;
    int q = fin_mapq(P, C.score, sub, C.csub, l, C.seedcov, C.sub_n);
    if (q < 0) return -1;
    q = q > q_pe ? q : q_pe < q + 40 ? q_pe : q + 40;                 // (:294-295)
    const int cap = pair_raw_mapq(C.score - C.csub, P.a);             // (:298-299)
    return q < cap ? q : cap;
}

__device__ __forceinline__ int pair_first_mapq(const PairParams& P, const AlnReg* L) {   // (:302-303)
    const AlnReg C = L[0];
    const int64_t rl = C.re - C.rb;
    const int l = (int64_t)(C.qe - C.qb) > rl ? C.qe - C.qb : (int)rl;
    return fin_mapq(P, C.score, C.sub, C.csub, l, C.seedcov, C.sub_n);
}

// the decision of mem_sam_pe (:268-304, :321-326), by one lane.  ran: mem_pair was called
// (both ends have regions, no MEM_F_NOPAIRING) and returned o, subo, n_sub, z; multi: :271-276.
__device__ void pair_decide(const PairParams& P, uint32_t p, const AlnReg* A0, int n0, const AlnReg* A1, int n1,
                            bool ran, int o, int subo, int n_sub, int z0, int z1, bool multi) {
    PairSel S;
    S.status = 0, S.branch = 0, S.z[0] = S.z[1] = 0, S.mapq[0] = S.mapq[1] = -1, S.proper = 0;
    S.o = ran ? o : 0, S.subo = ran ? subo : 0, S.n_sub = ran ? n_sub : 0;
    S.sub[0] = S.sub[1] = 0, S.promoted[0] = S.promoted[1] = 0;
    bool host = false;
    if (ran && o > 0 && !multi) {
        const int score_un = A0[0].score + A1[0].score - P.pen_unpaired;   // (:278)
        const int so = subo > score_un ? subo : score_un;                  // (:280)
        int q_pe = pair_raw_mapq(o - so, P.a);
        if (n_sub > 0) {
            if (n_sub >= FIN_TAB_LEN) host = true;
            else q_pe -= P.subn_tab[n_sub];                                // (:282)
        }
        if (q_pe < 0) q_pe = 0;
        if (q_pe > 60) q_pe = 60;
        if (!host && o > score_un) {                                       // (:286-299)
            S.branch = 1, S.z[0] = z0, S.z[1] = z1, S.proper = 2;
            S.mapq[0] = pair_end_mapq(P, A0, z0, q_pe, S.sub[0], S.promoted[0]);
            S.mapq[1] = pair_end_mapq(P, A1, z1, q_pe, S.sub[1], S.promoted[1]);
            host = S.mapq[0] < 0 || S.mapq[1] < 0;
        } else if (!host) {                                                // (:300-304)
            S.branch = 2;
            S.mapq[0] = pair_first_mapq(P, A0);
            S.mapq[1] = pair_first_mapq(P, A1);
            host = S.mapq[0] < 0 || S.mapq[1] < 0;
        }
    } else if (!P.nopairing && n0 > 0 && n1 > 0 && A0[0].score >= P.T && A1[0].score >= P.T) {   // (:321-325)
        int64_t dist;
        const PairDir D = P.dirs[pe_infer_dir(P.l_pac, A0[0].rb, A1[0].rb, dist)];
        if (!D.failed && dist >= (int64_t)D.low && dist <= (int64_t)D.high) S.proper = 2;
    }
    if (host) {
        S.status = PAIR_HOST, S.branch = 0, S.z[0] = S.z[1] = 0, S.mapq[0] = S.mapq[1] = 0, S.proper = 0;
        S.o = S.subo = S.n_sub = 0, S.sub[0] = S.sub[1] = 0, S.promoted[0] = S.promoted[1] = 0;
    }
    P.sel[p] = S;
}

// z[] of the best candidate (:226-228): by = k << 32 | i, two positions of v of opposite ends
template <int S>
__device__ __forceinline__ void pair_best_z(const Keys<S>& K, uint64_t by, int& z0, int& z1) {
    const uint64_t ya = K.Y((int)(by >> 32)), yb = K.Y((int)(uint32_t)by);
    const int ia = (int)((uint32_t)ya >> 2), ib = (int)((uint32_t)yb >> 2);
    z0 = (ya & 1) ? ib : ia;
    z1 = (ya & 1) ? ia : ib;
}

// ------------------------------------------------------------- lane tier
__global__ __launch_bounds__(64) void pair_lane_kernel(PairParams P) {
    __shared__ __attribute__((aligned(16))) uint64_t lds[2 * PAIR_LANE_MAX * 64];
    const uint32_t t = blockIdx.x * 64u + threadIdx.x;
    if (t >= P.ctr[0]) return;
    const uint32_t p = P.lane_list[t];
    const uint64_t b0 = P.reg_off[2 * p], b1 = P.reg_off[2 * p + 1];
    const int n0 = (int)(b1 - b0), n1 = (int)(P.reg_off[2 * p + 2] - b1);
    const AlnReg* A0 = P.regs + b0;
    const AlnReg* A1 = P.regs + b1;
    const bool ran = !P.nopairing && n0 > 0 && n1 > 0;
    int o = 0, sub = 0, n_sub = 0, z0 = 0, z1 = 0;
    bool multi = false;
    if (ran) {
        Keys<64> K;
        K.x = lds + threadIdx.x, K.y = lds + PAIR_LANE_MAX * 64 + threadIdx.x;
        const int n = n0 + n1;
        for (int j = 0; j < n; ++j) {   // insert each key at its place
            uint64_t x, y;
            if (j < n0) pair_key(A0[j], P.l_pac, j, 0, x, y);
            else pair_key(A1[j - n0], P.l_pac, j - n0, 1, x, y);
            int at = j;
            for (; at > 0 && pair_gt(K.X(at - 1), K.Y(at - 1), x, y); --at) K.X(at) = K.X(at - 1), K.Y(at) = K.Y(at - 1);
            K.X(at) = x, K.Y(at) = y;
        }
        const uint64_t idx = pair_id_bits(P, p);
        const int tmp = pair_tmp(P);
        Acc A = {0, 0, 0, 0};
        uint32_t cnt = 0;
        for (int i = 1; i < n; ++i) pair_scan<64, false>(P, K, i, idx, 0, tmp, A, cnt);
        if (A.n) {
            o = (int)(A.bx >> 32);
            sub = A.n > 1 ? A.sub : 0;                                           // (:230)
            for (int i = 1; i < n; ++i) pair_scan<64, true>(P, K, i, idx, sub, tmp, A, cnt);
            n_sub = A.n > 1 ? (int)cnt - 1 : 0;                                  // (:231-232): all but the best
            pair_best_z(K, A.by, z0, z1);
        }
        for (int j = 1; j < n0 && !multi; ++j) multi = A0[j].secondary < 0 && A0[j].score >= P.T;   // (:271-275)
        for (int j = 1; j < n1 && !multi; ++j) multi = A1[j].secondary < 0 && A1[j].score >= P.T;
    }
    pair_decide(P, p, A0, n0, A1, n1, ran, o, sub, n_sub, z0, z1, multi);
}

// ------------------------------------------------------------- wave tier
__device__ void pair_one_wave(const PairParams& P, uint8_t* lds, Acc* racc, uint32_t* rcnt, uint32_t p, int lane) {
    const uint64_t b0 = P.reg_off[2 * p], b1 = P.reg_off[2 * p + 1];
    const int n0 = (int)(b1 - b0), n1 = (int)(P.reg_off[2 * p + 2] - b1);
    const AlnReg* A0 = P.regs + b0;
    const AlnReg* A1 = P.regs + b1;
    const bool ran = !P.nopairing && n0 > 0 && n1 > 0;
    int o = 0, sub = 0, n_sub = 0, z0 = 0, z1 = 0;
    bool multi = false;
    if (ran) {
        Keys<1> K;
        K.x = reinterpret_cast<uint64_t*>(lds), K.y = reinterpret_cast<uint64_t*>(lds) + PAIR_MAX_KEYS;
        const int n = n0 + n1;
        int m = 2;
        while (m < n) m <<= 1;   // n <= PAIR_MAX_KEYS, a power of two
        bool mine = false;
        for (int j = lane; j < m; j += 64) {
            uint64_t x = ~0ull, y = ~0ull;   // padding sorts behind every key (x < 2^63)
            if (j < n0) {
                pair_key(A0[j], P.l_pac, j, 0, x, y);
                mine = mine || (j > 0 && A0[j].secondary < 0 && A0[j].score >= P.T);
            } else if (j < n) {
                pair_key(A1[j - n0], P.l_pac, j - n0, 1, x, y);
                mine = mine || (j > n0 && A1[j - n0].secondary < 0 && A1[j - n0].score >= P.T);
            }
            K.X(j) = x, K.Y(j) = y;
        }
        multi = __ballot(mine) != 0;   // (:271-275)
        __syncthreads();
        for (int k = 2; k <= m; k <<= 1) {   // bitonic network, ascending
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = lane; t < m; t += 64) {
                    const int l = t ^ j;
                    if (l > t) {
                        const uint64_t ax = K.X(t), ay = K.Y(t), bx = K.X(l), by = K.Y(l);
                        if (pair_gt(ax, ay, bx, by) == ((t & k) == 0)) K.X(t) = bx, K.Y(t) = by, K.X(l) = ax, K.Y(l) = ay;
                    }
                }
                __syncthreads();
            }
        }
        const uint64_t idx = pair_id_bits(P, p);
        const int tmp = pair_tmp(P);
        Acc A = {0, 0, 0, 0};
        uint32_t cnt = 0;
        for (int i = lane; i < n; i += 64) pair_scan<1, false>(P, K, i, idx, 0, tmp, A, cnt);
        racc[lane] = A;
        __syncthreads();
        if (lane == 0)
            for (int l = 1; l < 64; ++l) acc_merge(A, racc[l]);
        if (lane == 0) racc[0] = A;
        __syncthreads();
        A = racc[0];
        if (A.n) {
            o = (int)(A.bx >> 32);
            sub = A.n > 1 ? A.sub : 0;                                           // (:230)
            for (int i = lane; i < n; i += 64) pair_scan<1, true>(P, K, i, idx, sub, tmp, A, cnt);
            rcnt[lane] = cnt;
            __syncthreads();
            if (lane == 0) {
                uint32_t c = 0;
                for (int l = 0; l < 64; ++l) c += rcnt[l];
                n_sub = A.n > 1 ? (int)c - 1 : 0;                                // (:231-232): all but the best
            }
            pair_best_z(K, A.by, z0, z1);
        }
    }
    if (lane == 0) pair_decide(P, p, A0, n0, A1, n1, ran, o, sub, n_sub, z0, z1, multi);
}

__global__ __launch_bounds__(64) void pair_wave_kernel(PairParams P) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[PAIR_LDS_BYTES];
    __shared__ Acc racc[64];
    __shared__ uint32_t rcnt[64];
    const uint32_t n = P.ctr[1];
    for (uint32_t w = blockIdx.x; w < n; w += gridDim.x) {
        pair_one_wave(P, lds, racc, rcnt, P.wave_list[w], (int)threadIdx.x);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void pair_split_kernel(PairParams P) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= (uint32_t)P.n_pairs) return;
    const uint64_t n0 = P.reg_off[2 * p + 1] - P.reg_off[2 * p], n1 = P.reg_off[2 * p + 2] - P.reg_off[2 * p + 1];
    if (n0 > (uint64_t)FIN_MAX_REGS || n1 > (uint64_t)FIN_MAX_REGS) {
        PairSel S;
        S.status = PAIR_HOST, S.branch = 0, S.z[0] = S.z[1] = 0, S.mapq[0] = S.mapq[1] = 0, S.proper = 0;
        S.o = S.subo = S.n_sub = 0, S.sub[0] = S.sub[1] = 0, S.promoted[0] = S.promoted[1] = 0;
        P.sel[p] = S;
    } else if (n0 + n1 <= (uint64_t)PAIR_LANE_MAX) {
        P.lane_list[atomicAdd(&P.ctr[0], 1u)] = p;
    } else {
        P.wave_list[atomicAdd(&P.ctr[1], 1u)] = p;
    }
}

}  // namespace
}  // namespace smem

extern "C" hipError_t smem_launch_pst(const smem::PstParams* P, int n_cu, hipStream_t st) {
    if (P->n_pairs <= 0) return hipSuccess;
    const int slots = n_cu * smem::PST_WAVES_PER_CU / 4, need = (P->n_pairs + 255) / 256;
    hipLaunchKernelGGL(smem::pst_kernel, dim3((unsigned)(need < slots ? need : slots)), dim3(256), 0, st, *P);
    return hipGetLastError();
}

extern "C" hipError_t smem_launch_pair_split(const smem::PairParams* P, hipStream_t st) {
    if (P->n_pairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(smem::pair_split_kernel, dim3((unsigned)((P->n_pairs + 255) / 256)), dim3(256), 0, st, *P);
    return hipGetLastError();
}

extern "C" hipError_t smem_launch_pair_lane(const smem::PairParams* P, hipStream_t st) {
    if (P->n_pairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(smem::pair_lane_kernel, dim3((unsigned)((P->n_pairs + 63) / 64)), dim3(64), 0, st, *P);
    return hipGetLastError();
}

extern "C" hipError_t smem_launch_pair_wave(const smem::PairParams* P, int n_cu, hipStream_t st) {
    if (P->n_pairs <= 0) return hipSuccess;
    const int slots = n_cu * smem::PAIR_WAVES_PER_CU;
    hipLaunchKernelGGL(smem::pair_wave_kernel, dim3((unsigned)(P->n_pairs < slots ? P->n_pairs : slots)), dim3(64), 0, st,
                       *P);
    return hipGetLastError();
}
