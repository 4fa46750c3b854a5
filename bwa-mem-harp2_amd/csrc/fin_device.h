// What the region stages share (fin_kernels.hip, matesw_kernels.hip, pair_kernels.hip): one
// read's regions as a view in LDS, ks_introsort and its parts comparison for comparison over a
// permutation, the redundancy test and mem_sort_and_dedup by one wave, hash_64, mem_infer_dir and
// mem_approx_mapq_se.  All three files are compiled with -ffp-contract=off (see fin_kernels.hip).
#pragma once
#include "fin_kernels.h"

namespace smem {
namespace {

constexpr int FIN_STK = 16;  // pending introsort segments: log2(FIN_MAX_REGS / 16) + 1 = 7 at most

__device__ __forceinline__ uint64_t fin_hash_64(uint64_t key) {  // software/utils.h:99-110
    key += ~(key << 32);
    key ^= (key >> 22);
    key += ~(key << 13);
    key ^= (key >> 8);
    key += (key << 3);
    key ^= (key >> 15);
    key += ~(key << 27);
    key ^= (key >> 31);
    return key;
}

// mem_infer_dir (software/bwamem_pair.c:23-30)
__device__ __forceinline__ int pe_infer_dir(int64_t l_pac, int64_t b1, int64_t b2, int64_t& dist) {
    const int r1 = b1 >= l_pac, r2 = b2 >= l_pac;
    const int64_t p2 = r1 == r2 ? b2 : (l_pac << 1) - 1 - b2;
    dist = p2 > b1 ? p2 - b1 : b1 - p2;
    return (r1 == r2 ? 0 : 1) ^ (p2 > b1 ? 0 : 3);
}

// One read's regions in LDS, element i of an array at [i * S]: S = 1 for the
// wave tier (the block holds one read), S = 64 for the lane tier (the pointers
// start at the lane's own column).  Indexed by region -- the position in the
// read's raw list -- except perm, which is the array a[] of the reference:
// perm[i] is the region at position i.
template <int S>
struct View {
    int64_t* ka;     // re; the hash once the second sort is done
    int64_t* kb;     // rb; then re - rb in its low word
    int32_t* qb;
    int32_t* qe;
    int32_t* score;
    int32_t* sub;
    uint32_t* perm;
    uint32_t* aux;   // secondary + 1 in the low 16 bits, the increments of sub_n above
    __device__ __forceinline__ int64_t& KA(uint32_t x) const { return ka[x * S]; }
    __device__ __forceinline__ int64_t& KB(uint32_t x) const { return kb[x * S]; }
    __device__ __forceinline__ int32_t& RLEN(uint32_t x) const { return reinterpret_cast<int32_t*>(kb + x * S)[0]; }
    __device__ __forceinline__ int32_t& QB(uint32_t x) const { return qb[x * S]; }
    __device__ __forceinline__ int32_t& QE(uint32_t x) const { return qe[x * S]; }
    __device__ __forceinline__ int32_t& SC(uint32_t x) const { return score[x * S]; }
    __device__ __forceinline__ int32_t& SUB(uint32_t x) const { return sub[x * S]; }
    __device__ __forceinline__ uint32_t& AUX(uint32_t x) const { return aux[x * S]; }
    __device__ __forceinline__ uint32_t& P(uint32_t i) const { return perm[i * S]; }
};

template <int S>
__device__ __forceinline__ View<S> make_view(uint8_t* lds, int col) {
    View<S> v;
    v.ka = reinterpret_cast<int64_t*>(lds) + col;
    v.kb = reinterpret_cast<int64_t*>(lds + 8 * FIN_MAX_REGS) + col;
    v.qb = reinterpret_cast<int32_t*>(lds + 16 * FIN_MAX_REGS) + col;
    v.qe = reinterpret_cast<int32_t*>(lds + 20 * FIN_MAX_REGS) + col;
    v.score = reinterpret_cast<int32_t*>(lds + 24 * FIN_MAX_REGS) + col;
    v.sub = reinterpret_cast<int32_t*>(lds + 28 * FIN_MAX_REGS) + col;
    v.perm = reinterpret_cast<uint32_t*>(lds + 32 * FIN_MAX_REGS) + col;
    v.aux = reinterpret_cast<uint32_t*>(lds + 36 * FIN_MAX_REGS) + col;
    return v;
}

// the orders of mem_sort_and_dedup (software/bwamem.c:696-703), over regions; the third, by hash, is fin_kernels.hip's
template <int S>
struct LtRe {
    View<S> v;
    __device__ __forceinline__ bool operator()(uint32_t x, uint32_t y) const { return v.KA(x) < v.KA(y); }
};
template <int S>
struct LtScore {
    View<S> v;
    __device__ __forceinline__ bool operator()(uint32_t x, uint32_t y) const {
        const int sx = v.SC(x), sy = v.SC(y);
        if (sx != sy) return sx > sy;
        const int64_t bx = v.KB(x), by = v.KB(y);
        return bx < by || (bx == by && v.QB(x) < v.QB(y));
    }
};
// __ks_insertsort over positions [s, t)
template <int S, class LT>
__device__ __forceinline__ void fin_insertsort(const View<S>& v, uint32_t s, uint32_t t, const LT& lt) {
    for (uint32_t i = s + 1; i < t; ++i) {
        const uint32_t x = v.P(i);
        uint32_t j = i;
        for (; j > s; --j) {
            const uint32_t y = v.P(j - 1);
            if (!lt(x, y)) break;
            v.P(j) = y;
        }
        if (j != i) v.P(j) = x;
    }
}

// ks_combsort over positions [s, s + n)
template <int S, class LT>
__device__ void fin_combsort(const View<S>& v, uint32_t s, uint32_t n, const LT& lt) {
    const double shrink = 1.2473309501039786540366528676643;
    uint32_t gap = n;
    bool swapped;
    do {
        if (gap > 2) {
            gap = (uint32_t)((double)gap / shrink);
            if (gap == 9 || gap == 10) gap = 11;
        }
        swapped = false;
        for (uint32_t i = s; i + gap < s + n; ++i) {
            const uint32_t x = v.P(i), y = v.P(i + gap);
            if (lt(y, x)) {
                v.P(i) = y;
                v.P(i + gap) = x;
                swapped = true;
            }
        }
    } while (swapped || gap > 2);
    if (gap != 1) fin_insertsort(v, s, s + n, lt);
}

// ks_introsort of positions [0, n), comparison for comparison.  SMALL (n <=
// FIN_LANE_MAX = 16): no segment is ever pushed (only those longer than 16 are)
// and the depth budget of 2 * ceil(log2 n) >= 4 outlasts the single partition,
// so neither the stack nor the combsort exists; else stk holds the pending
// segments, 3 words each, in LDS.
template <bool SMALL, int S, class LT>
__device__ void fin_introsort(const View<S>& v, uint32_t n, const LT& lt, uint32_t* stk) {
    if (n < 1) return;
    if (n == 2) {
        const uint32_t x = v.P(0), y = v.P(1);
        if (lt(y, x)) v.P(0) = y, v.P(1) = x;
        return;
    }
    int d = 2, top = 0;
    while ((1u << d) < n) ++d;
    d <<= 1;
    uint32_t s = 0, t = n - 1;
    for (;;) {
        if (s < t) {
            if (--d == 0) {
                if (!SMALL) fin_combsort(v, s, t - s + 1, lt);
                t = s;
                continue;
            }
            uint32_t i = s, j = t, k = i + ((j - i) >> 1) + 1;
            {
                const uint32_t xi = v.P(i), xj = v.P(j), xk = v.P(k);
                if (lt(xk, xi)) {
                    if (lt(xk, xj)) k = j;
                } else {
                    k = lt(xj, xi) ? i : j;
                }
            }
            const uint32_t rp = v.P(k);
            if (k != t) v.P(k) = v.P(t), v.P(t) = rp;
            for (;;) {
                do ++i;
                while (lt(v.P(i), rp));
                do --j;
                while (i <= j && lt(rp, v.P(j)));
                if (j <= i) break;
                const uint32_t x = v.P(i);
                v.P(i) = v.P(j);
                v.P(j) = x;
            }
            {
                const uint32_t x = v.P(i);
                v.P(i) = v.P(t);
                v.P(t) = x;
            }
            if (i - s > t - i) {
                if (!SMALL && i - s > 16 && top < FIN_STK) {
                    stk[3 * top] = s, stk[3 * top + 1] = i - 1, stk[3 * top + 2] = (uint32_t)d;
                    ++top;
                }
                s = t - i > 16 ? i + 1 : t;
            } else {
                if (!SMALL && t - i > 16 && top < FIN_STK) {
                    stk[3 * top] = i + 1, stk[3 * top + 1] = t, stk[3 * top + 2] = (uint32_t)d;
                    ++top;
                }
                t = i - s > 16 ? i - 1 : s;
            }
        } else {
            if (top == 0) {
                fin_insertsort(v, 0, n, lt);
                return;
            }
            --top;
            s = stk[3 * top], t = stk[3 * top + 1], d = (int)stk[3 * top + 2];
        }
    }
}

// "one of the hits is redundant" (software/bwamem.c:717-721): float products
__device__ __forceinline__ bool fin_redundant(float mlr, int64_t prb, int64_t pre, int pqb, int pqe, int64_t qrb,
                                              int64_t qre, int qqb, int qqe) {
#pragma clang fp contract(off)
    const int64_t orr = qre - prb;
    const int64_t oq = qqb < pqb ? qqe - pqb : pqe - qqb;
    const int64_t mr = qre - qrb < pre - prb ? qre - qrb : pre - prb;
    const int64_t mq = qqe - qqb < pqe - pqb ? qqe - qqb : pqe - pqb;
    return (float)orr > mlr * (float)mr && (float)oq > mlr * (float)mq;
}

// mem_approx_mapq_se (software/bwamem.c:1333-1356); -1 where a table ends or l < 1.  PT: FinParams, or
// the pairing stage's parameters, which carry the same options and tables under the same names
template <class PT>
__device__ int fin_mapq(const PT& P, int score, int sub0, int csub, int l, int seedcov, int sub_n) {
#pragma clang fp contract(off)
    int sub = sub0 ? sub0 : P.min_seed_len * P.a;
    sub = csub > sub ? csub : sub;
    if (sub >= score) return 0;
    if (l < 1) return -1;
    const double identity = 1. - (double)(l * P.a - score) / (double)(P.a + P.b) / (double)l;
    int mapq;
    if (score == 0) {
        mapq = 0;
    } else if (P.mapQ_coef_len > 0.f) {
        double tmp;
        if ((float)l < P.mapQ_coef_len) {
            tmp = 1.;
        } else {
            if (l < 2 || l >= FIN_TAB_LEN) return -1;
            tmp = (double)P.mapQ_coef_fac / P.log_tab[l];
        }
        const double id2 = identity * identity;
        tmp = tmp * id2;
        double x = 6.02 * (double)(score - sub);
        x = x / (double)P.a;
        x = x * tmp;
        x = x * tmp;
        x = x + .499;
        mapq = (int)x;
    } else {
        if (seedcov < 1 || seedcov >= FIN_TAB_LEN) return -1;
        double x = 1. - (double)sub / (double)score;
        x = 30.0 * x;
        x = x * P.log_tab[seedcov];
        x = x + .499;
        mapq = (int)x;
        if (identity < 0.95) {
            double y = (double)mapq * identity;
            y = y * identity;
            y = y + .499;
            mapq = (int)y;
        }
    }
    if (sub_n > 0) {
        if (sub_n >= FIN_TAB_LEN) return -1;
        mapq -= P.subn_tab[sub_n];
    }
    if (mapq > 60) mapq = 60;
    if (mapq < 0) mapq = 0;
    return mapq;
}

// keep the positions of [from, n) whose region passes `keep`, in order, behind [0, from);
// in place: a chunk is read before it is written, and writes never pass the chunk
template <class KEEP>
__device__ uint32_t fin_compact_wave(const View<1>& v, uint32_t from, uint32_t n, int lane, const KEEP& keep) {
    uint32_t m = from;
    const uint64_t below = (1ull << lane) - 1;
    for (uint32_t b = from; b < n; b += 64) {
        const uint32_t k = b + (uint32_t)lane;
        const uint32_t x = k < n ? v.P(k) : 0u;
        const bool kp = k < n && keep(k, x);
        const uint64_t mask = __ballot(kp);
        __syncthreads();
        if (kp) v.P(m + (uint32_t)__builtin_popcountll(mask & below)) = x;
        m += (uint32_t)__builtin_popcountll(mask);
        __syncthreads();
    }
    return m;
}

// mem_sort_and_dedup (software/bwamem.c:705-746) of the n > 1 regions a wave tier view holds, by
// the one wave of its block: the kept regions' count, their order in v.P
[[maybe_unused]] __device__ uint32_t fin_sort_dedup_wave(const View<1>& v, uint32_t n, float mlr, uint32_t* stk, int lane) {
    if (lane == 0) fin_introsort<false>(v, n, LtRe<1>{v}, stk);
    __syncthreads();
    for (uint32_t i = 1; i < n; ++i) {
        const uint32_t p = v.P(i);
        const int64_t prb = v.KB(p), pre = v.KA(p);
        if (prb >= v.KA(v.P(i - 1))) continue;
        const int pqb = v.QB(p), pqe = v.QE(p), psc = v.SC(p);
        // candidates j = i - 1 downwards, 64 a pass: the loop ends at the first j with
        // rb >= a[j].re or at the first redundant j that beats p; every redundant j
        // before that is excluded.  Whether a[j] is already excluded was settled by
        // earlier i: within one i every j is looked at once.
        for (int hi = (int)i - 1; hi >= 0; hi -= 64) {
            const int j = hi - lane;
            bool in = j >= 0, red = false, stop = false;
            uint32_t q = 0;
            int qqb = 0;
            if (in) {
                q = v.P((uint32_t)j);
                const int64_t qre = v.KA(q);
                in = prb < qre;
                if (in) {
                    qqb = v.QB(q);
                    const int qqe = v.QE(q);
                    red = qqe != qqb && fin_redundant(mlr, prb, pre, pqb, pqe, v.KB(q), qre, qqb, qqe);
                    stop = red && psc < v.SC(q);
                }
            }
            const uint64_t m_out = __ballot(!in);
            const int f = m_out ? __builtin_ctzll(m_out) : 64;   // lanes below f are inside the loop
            const uint64_t inside = f == 64 ? ~0ull : (1ull << f) - 1;
            const uint64_t m_stop = __ballot(stop) & inside;
            const int s = m_stop ? __builtin_ctzll(m_stop) : 64;
            if (red && lane < f && lane < s) v.QE(q) = qqb;
            if (s < 64 && lane == s) v.QE(p) = pqb;
            if (f < 64 || s < 64) break;
        }
        __syncthreads();
    }
    uint32_t m = fin_compact_wave(v, 0, n, lane, [&](uint32_t, uint32_t x) { return v.QE(x) > v.QB(x); });
    if (m == 0) {
        n = 1;  // the reference's second pass starts its count at 1 (software/bwamem.c:740)
    } else {
        n = m;
        if (lane == 0) fin_introsort<false>(v, n, LtScore<1>{v}, stk);
        __syncthreads();
        // "mark identical hits" compares fields the marking does not touch
        n = fin_compact_wave(v, 1, n, lane, [&](uint32_t k, uint32_t x) {
            const uint32_t y = v.P(k - 1);
            return !(v.SC(x) == v.SC(y) && v.KB(x) == v.KB(y) && v.QB(x) == v.QB(y));
        });
    }
    return n;
}

}  // namespace
}  // namespace smem
