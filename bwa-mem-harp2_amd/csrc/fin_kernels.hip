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
// libm; the division by log(l) is an IEEE division on both sides.
#include "fin_kernels.h"

namespace smem {
namespace {

constexpr int FIN_STK = 16;  // pending introsort segments: log2(FIN_MAX_REGS / 16) + 1 = 7 at most

__device__ __forceinline__ uint64_t hash_64(uint64_t key) {  // software/utils.h:99-110
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

// the three orders (software/bwamem.c:696-703), over regions
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
template <int S>
struct LtHash {
    View<S> v;
    __device__ __forceinline__ bool operator()(uint32_t x, uint32_t y) const {
        const int sx = v.SC(x), sy = v.SC(y);
        return sx > sy || (sx == sy && (uint64_t)v.KA(x) < (uint64_t)v.KA(y));
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

// "significant overlap" on the query (software/bwamem.c:770-774)
__device__ __forceinline__ bool fin_overlaps(float ml, int jqb, int jqe, int iqb, int iqe) {
#pragma clang fp contract(off)
    const int b_max = jqb > iqb ? jqb : iqb;
    const int e_min = jqe < iqe ? jqe : iqe;
    if (e_min <= b_max) return false;
    const int min_l = iqe - iqb < jqe - jqb ? iqe - iqb : jqe - jqb;
    return (float)(e_min - b_max) >= (float)min_l * ml;
}

// mem_approx_mapq_se (software/bwamem.c:1333-1356); -1 where a table ends or l < 1
__device__ int fin_mapq(const FinParams& P, int score, int sub0, int csub, int l, int seedcov, int sub_n) {
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
            v.KA(x) = (int64_t)hash_64((uint64_t)(A.id + (int64_t)k));
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
    if (n > 1) {  // mem_sort_and_dedup
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
                        red = qqe != qqb && fin_redundant(P.mask_level_redun, prb, pre, pqb, pqe, v.KB(q), qre, qqb, qqe);
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
    }
    // mem_test_and_remove_exact
    if (P.no_exact && n > 0 && P.regs[A.base + v.P(0)].truesc == A.qlen * P.a) v.perm += 1, --n;
    uint32_t n_sel = 0;
    if (n > 0) {  // mem_mark_primary_se
        for (uint32_t k = (uint32_t)lane; k < n; k += 64) {
            const uint32_t x = v.P(k);
            const int rlen = (int)(v.KA(x) - v.KB(x));
            v.KA(x) = (int64_t)hash_64((uint64_t)(A.id + (int64_t)k));
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
