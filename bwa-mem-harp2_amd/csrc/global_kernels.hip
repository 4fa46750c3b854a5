// Regions -> alignments on gfx950: the alignment part of mem_reg2aln
// (software/bwamem.c:1504-1547) -- the band from infer_bw, up to three
// bwa_gen_cigar2 calls (software/bwa.c:96-179) with a doubled band, each a
// banded global alignment with traceback (ksw_global2, software/ksw.c:501-584),
// then NM / MD, the squeeze of a leading or trailing deletion and the clips.
//
// One lane group (16, 32 or 64 lanes) per region; a group walks the target
// rows in order and its lanes hold the band's columns, G at a time.  The
// reference separates M from H: F(i,j+1) = max(M(i,j) - oe_ins, F(i,j) - e_ins)
// with M(i,j) = H(i-1,j-1) + S(i,j), so a row's M values depend on the previous
// row only and
//     F(i,j) = max_{beg <= k < j} (M(i,k) - oe_ins + k e_ins) - (j - 1) e_ins,
// an exclusive prefix max across the lanes (DPP row steps, carried from one
// pass of G columns to the next).  E and H are element-wise.  All values are
// exact integers and the direction bits come from the reference's own
// comparisons (m >= e, h >= f, e > t, f > t), so ties fall as they do there.
// The reference's column array (H of the previous row one column to the left,
// E of this row) lives in LDS with the query and the target; the direction
// matrix (n_col x tlen, 4 bits a cell: 2 bits H's source, the E and F
// extension bits) follows it in LDS when it fits the group's share and else
// goes to a scratch slab in HBM (the one-region-per-wave launch).  Only the
// last try is traced back: whether another try follows depends on the score
// alone.  Traceback, NM and MD are serial and run on the group's first lane;
// the run-length CIGAR is built in the column array's LDS (dead by then), MD
// is walked twice (length, then bytes) and output space is claimed from two
// cursors, which also give the sizes a too-small pool needs.
//
// g2a_prep_kernel (at the end) makes the tasks and the lane groups' lists on the
// device, for the host-buffer call and the resident batch stage alike; the
// lists' lengths stay in device memory, a region that defers appends itself to
// the scratch tier's list, and with a contig table the serial end also names
// the contig of the final position (bns_pos2rid, software/bwamem.c:1548).
#include "global_kernels.h"

namespace smem {
namespace {

constexpr int MINUS_INF = -0x40000000;  // software/ksw.c:487

__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

// every lane of a group belongs to one wave, whose LDS operations complete in
// order: only the compiler has to keep the phases apart
__device__ __forceinline__ void group_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// inclusive prefix max over the G lanes of a group (groups are aligned to DPP rows)
template <int G>
__device__ __forceinline__ int gscan_max(int v) {
    v = imax(v, __builtin_amdgcn_update_dpp(MINUS_INF, v, 0x111, 0xf, 0xf, false));  // row_shr:1
    v = imax(v, __builtin_amdgcn_update_dpp(MINUS_INF, v, 0x112, 0xf, 0xf, false));  // row_shr:2
    v = imax(v, __builtin_amdgcn_update_dpp(MINUS_INF, v, 0x114, 0xf, 0xf, false));  // row_shr:4
    v = imax(v, __builtin_amdgcn_update_dpp(MINUS_INF, v, 0x118, 0xf, 0xf, false));  // row_shr:8
    if (G >= 32) v = imax(v, __builtin_amdgcn_update_dpp(MINUS_INF, v, 0x142, 0xa, 0xf, false));  // row_bcast:15
    if (G >= 64) v = imax(v, __builtin_amdgcn_update_dpp(MINUS_INF, v, 0x143, 0xc, 0xf, false));  // row_bcast:31
    return v;
}
// the value of the lane to the left; the group's first lane takes `first`
template <int G>
__device__ __forceinline__ int gshr1(int v, int first, int lg) {
    if (G == 16) return __builtin_amdgcn_update_dpp(first, v, 0x111, 0xf, 0xf, false);  // row_shr:1
    const int s = __builtin_amdgcn_update_dpp(first, v, 0x138, 0xf, 0xf, false);        // wave_shr:1
    return lg == 0 ? first : s;
}
// the value of the group's last lane
template <int G>
__device__ __forceinline__ int glast(int v, int lane) {
    return __shfl(v, (lane & ~(G - 1)) | (G - 1));
}

__device__ __forceinline__ int pac_base(const uint8_t* pac, int64_t l) {
    return pac[l >> 2] >> ((~l & 3) << 1) & 3;  // _get_pac (software/bntseq.h)
}

// ksw_global2's DP (software/ksw.c:519-565) by one group: returns the score, fills z
template <int G>
__device__ __forceinline__ int global_dp(int lane, int qlen, int tlen, int w, const uint8_t* sq, const uint8_t* st,
                                         int2* eh, uint8_t* z, int row_bytes, const int8_t* mat, int o_del, int e_del,
                                         int o_ins, int e_ins) {
    const int lg = lane & (G - 1);
    const int oe_del = o_del + e_del, oe_ins = o_ins + e_ins;
    for (int j = lg; j <= qlen; j += G)  // the first row (software/ksw.c:519-522)
        eh[j] = make_int2(j == 0 ? 0 : j <= w ? -(o_ins + e_ins * j) : MINUS_INF, MINUS_INF);
    group_fence();
    for (int i = 0; i < tlen; ++i) {
        const int beg = i > w ? i - w : 0;
        const int end = i + w + 1 < qlen ? i + w + 1 : qlen;
        const int8_t* srow = mat + (int)st[i] * 5;
        uint8_t* zi = z + (size_t)i * row_bytes;
        int carry_p = MINUS_INF;                                          // prefix max of the passes before
        int carry_h = beg == 0 ? -(o_del + e_del * (i + 1)) : MINUS_INF;  // h1: H(i, beg - 1)
        for (int c0 = 0; beg + c0 < end; c0 += G) {
            const int c = c0 + lg, j = beg + c;
            const bool valid = j < end;
            int m = MINUS_INF, e = MINUS_INF;
            if (valid) {
                const int2 p = eh[j];
                m = p.x + srow[sq[j]];
                e = p.y;
            }
            const int incl = gscan_max<G>(valid ? m - oe_ins + c * e_ins : MINUS_INF);
            const int excl = imax(gshr1<G>(incl, MINUS_INF, lg), carry_p);
            // only the band's first column sees no F (every M is finite)
            const int f = c == 0 ? MINUS_INF : excl - (c - 1) * e_ins;
            int d = m >= e ? 0 : 1;
            int h = m >= e ? m : e;
            d = h >= f ? d : 2;
            h = h >= f ? h : f;
            int t = m - oe_del;
            int e2 = e - e_del;
            d |= e2 > t ? 4 : 0;
            e2 = e2 > t ? e2 : t;
            t = m - oe_ins;
            d |= f - e_ins > t ? 8 : 0;
            if (!valid) d = 0;
            const int hl = gshr1<G>(h, carry_h, lg);  // H(i, j - 1)
            const int dn = __builtin_amdgcn_update_dpp(0, d, 0x101, 0xf, 0xf, true);  // row_shl:1
            if (valid) {
                eh[j] = make_int2(hl, e2);
                if (j == end - 1) eh[end] = make_int2(h, MINUS_INF);
                if (!(lg & 1)) zi[c >> 1] = (uint8_t)(d | dn << 4);
            }
            if (beg + c0 + G < end) {  // another pass follows
                carry_p = imax(carry_p, glast<G>(incl, lane));
                carry_h = glast<G>(h, lane);
            }
        }
        group_fence();
    }
    return eh[qlen].x;
}

// NM and MD of bwa_gen_cigar2 (software/bwa.c:141-171) over the CIGAR stored
// last op first in rc[0 .. n): returns NM, emits the MD bytes
template <class Emit>
__device__ __forceinline__ int md_walk(const uint32_t* rc, int n, const uint8_t* sq, const uint8_t* st, bool rev,
                                       Emit emit) {
    auto base = [&](int c) { return rev ? "TGCAN"[c] : "ACGTN"[c]; };
    auto putw = [&](int u) {  // kputw of a non-negative number
        int div = 1;
        while (u / div >= 10) div *= 10;
        for (; div > 0; div /= 10) emit((char)('0' + u / div % 10));
    };
    int x = 0, y = 0, u = 0, n_mm = 0, n_gap = 0;
    for (int k = 0; k < n; ++k) {
        const int op = rc[n - 1 - k] & 0xf, len = (int)(rc[n - 1 - k] >> 4);
        if (op == 0) {
            for (int i = 0; i < len; ++i) {
                if (sq[x + i] != st[y + i]) {
                    putw(u);
                    emit(base(st[y + i]));
                    ++n_mm, u = 0;
                } else ++u;
            }
            x += len, y += len;
        } else if (op == 2) {
            if (k > 0 && k < n - 1) {  // not for a first or last deletion
                putw(u);
                emit('^');
                for (int i = 0; i < len; ++i) emit(base(st[y + i]));
                u = 0, n_gap += len;
            }
            y += len;
        } else if (op == 1) x += len, n_gap += len;
    }
    putw(u);
    return n_mm + n_gap;
}

// The serial end of a region on the group's first lane: traceback of the last try,
// NM / MD, squeeze, clips, and the claim of output space.
__device__ __forceinline__ void finish_region(const G2aParams& P, const G2aTask& T, int status, int score, int tries,
                                              bool dp, int w, int row_bytes, bool rev, int64_t fb, int2* eh,
                                              const uint8_t* sq, const uint8_t* st, const uint8_t* z) {
    const int qlen = T.qlen, tlen = (int)(T.re - T.rb);
    Aln A;
    A.pos = -1, A.is_rev = 0, A.n_cigar = 0, A.NM = 0, A.score = 0, A.tries = 0, A.status = status;
    A.cigar_off = 0, A.md_off = 0, A.md_len = 0, A.pad = 0;
    if (status == G2A_DEFERRED) {
        // the scratch-tier launch redoes it: onto that launch's list, with the matrix it may need
        atomicAdd(&P.cur[2], 1ull);
        const uint32_t slot = atomicAdd(&P.cnt[G2A_N_BIG], 1u);
        if (slot < P.defer_cap) P.defer[slot] = T.out;
        atomicMax(&P.cur[3], (unsigned long long)g2a_scratch_need(qlen, tlen, P.mat[0], P.o_del, P.e_del, P.o_ins,
                                                                  P.e_ins));
    }
    if (status == G2A_OK) {
        // the CIGAR last op first, in the column array's LDS: at most 2 qlen + 1 runs
        uint32_t* rc = reinterpret_cast<uint32_t*>(eh);
        const int rc_cap = 2 * (qlen + 1);
        int n = 0;
        bool bad = false;
        auto push = [&](int op, int len) {  // push_cigar (software/ksw.c:489-499)
            if (n == 0 || (int)(rc[n - 1] & 0xf) != op) {
                if (n < rc_cap) rc[n++] = (uint32_t)len << 4 | (uint32_t)op;
                else bad = true;
            } else rc[n - 1] += (uint32_t)len << 4;
        };
        if (!dp) push(0, qlen);
        else {  // backtrack (software/ksw.c:566-577)
            const int n_col = qlen < 2 * w + 1 ? qlen : 2 * w + 1;
            int which = 0, i = tlen - 1, k = (i + w + 1 < qlen ? i + w + 1 : qlen) - 1;
            while (i >= 0 && k >= 0) {
                const int col = k - (i > w ? i - w : 0);
                if (col < 0 || col >= n_col) {
                    bad = true;
                    break;
                }
                const int cell = z[(size_t)i * row_bytes + (col >> 1)] >> ((col & 1) << 2) & 0xf;
                which = which == 0 ? (cell & 3) : which == 1 ? (cell >> 2 & 1) : (cell >> 3 & 1) << 1;
                if (which == 0) push(0, 1), --i, --k;
                else if (which == 1) push(2, 1), --i;
                else push(1, 1), --k;
            }
            if (!bad) {
                if (i >= 0) push(2, i + 1);
                if (k >= 0) push(1, k + 1);
            }
        }
        if (bad) A.status = G2A_BADTRACE;
        else {
            int md_len = 0;
            A.NM = md_walk(rc, n, sq, st, rev, [&](char) { ++md_len; });
            A.score = score, A.tries = tries, A.is_rev = rev ? 1 : 0, A.md_len = md_len;
            // bns_depos of rb, or of re - 1 on the reverse strand (software/bwamem.c:1521)
            int64_t pos = fb;
            // squeeze out a leading, else a trailing deletion (software/bwamem.c:1523-1532)
            int first = 0, cnt = n;  // ops first .. first + cnt of the forward CIGAR
            if ((rc[n - 1] & 0xf) == 2) pos += rc[n - 1] >> 4, first = 1, --cnt;
            else if ((rc[0] & 0xf) == 2) --cnt;
            // the clips (software/bwamem.c:1533-1547)
            const int qe = T.qb + qlen;
            const int clip5 = rev ? T.l_query - qe : T.qb, clip3 = rev ? T.qb : T.l_query - qe;
            const int n_out = cnt + (clip5 ? 1 : 0) + (clip3 ? 1 : 0);
            A.pos = pos, A.n_cigar = n_out;
            A.cigar_off = atomicAdd(&P.cur[0], (unsigned long long)n_out);
            A.md_off = atomicAdd(&P.cur[1], (unsigned long long)md_len);
            if (A.cigar_off + (uint64_t)n_out <= P.cigar_cap) {
                uint32_t* o = P.cigar + A.cigar_off;
                if (clip5) *o++ = (uint32_t)clip5 << 4 | 3;
                for (int k = 0; k < cnt; ++k) *o++ = rc[n - 1 - first - k];
                if (clip3) *o++ = (uint32_t)clip3 << 4 | 3;
            }
            if (A.md_off + (uint64_t)md_len <= P.md_cap) {
                char* o = P.md + A.md_off;
                md_walk(rc, n, sq, st, rev, [&](char ch) { *o++ = ch; });
            }
        }
    }
    if (A.status == G2A_BADTRACE) atomicAdd(&P.cnt[G2A_N_BADTRACE], 1u);
    // the contig of the final position (software/bwamem.c:1548)
    if (P.rid) P.rid[T.out] = A.status == G2A_OK && P.ctg.off ? g2a_pos2rid(P.ctg.off, P.ctg.n, P.l_pac, A.pos) : -1;
    P.alns[T.out] = A;
}

// (registers capped for 4 waves a SIMD where the LDS allows as many: 8 KB a wave)
template <int G, int LDSB, bool BIG>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(BIG ? 1 : G == 16 ? 3 : 4)))
void g2a_kernel(G2aParams P) {
    constexpr int NG = 64 / G, B = LDSB / NG;
    __shared__ __attribute__((aligned(16))) uint8_t lds[LDSB];
    __shared__ int8_t smat[32];
    const int lane = (int)threadIdx.x, lg = lane & (G - 1), grp = lane / G;
    const uint32_t n = *P.n_dev;  // (the grid was sized from the host's upper bound)
    if (blockIdx.x * NG >= n) return;
    if (lane == 0)
        for (int k = 0; k < 25; ++k) smat[k] = P.mat[k];
    __syncthreads();
    uint8_t* const mine = lds + grp * B;
    for (uint32_t it = blockIdx.x * NG + grp; it < n; it += gridDim.x * NG) {
        group_fence();
        const G2aTask T = P.task[P.list[it]];
        const int qlen = T.qlen, tlen = (int)(T.re - T.rb);
        const bool rev = T.rb >= P.l_pac;
        // on the reverse strand bwa_gen_cigar2 reverses both sequences, so that gaps
        // land leftmost on the forward strand: the target is then the complement of
        // the forward strand read upwards from 2 l_pac - re (bns_get_seq, software/bntseq.c)
        const int64_t fb = rev ? 2 * P.l_pac - T.re : T.rb;
        const int fixed = g2a_fixed_bytes(qlen, tlen);
        int2* eh = reinterpret_cast<int2*>(mine);
        uint8_t* sq = mine + (qlen + 1) * 8;
        uint8_t* st = sq + ((qlen + 3) & ~3);
        uint8_t* zl = st + ((tlen + 3) & ~3);
        int status = G2A_OK, score = 0, tries = 0, w = 0, row_bytes = 0;
        bool dp = false;
        const uint8_t* z = nullptr;
        if (qlen < 1 || qlen > G2A_MAX_QLEN || tlen < 1 || tlen > G2A_MAX_TLEN) status = G2A_BADTRACE;
        else if (fixed > B) status = G2A_DEFERRED;
        if (status == G2A_OK) {
            for (int j = lg; j < qlen; j += G) sq[j] = P.codes[T.q_off + (uint64_t)(rev ? qlen - 1 - j : j)];
            for (int i = lg; i < tlen; i += G) st[i] = (uint8_t)(pac_base(P.pac, fb + i) ^ (rev ? 3 : 0));
            group_fence();
            // the band-doubling loop (software/bwamem.c:1504-1518)
            int w2 = g2a_first_w2(qlen, tlen, T.truesc, P.a, P.o_del, P.e_del, P.o_ins, P.e_ins, P.w, T.w);
            int last_sc = -(1 << 30);
            for (int i = 0;;) {
                ++tries;
                if (qlen == tlen && w2 == 0) {  // no gap, no DP (software/bwa.c:115-121)
                    dp = false;
                    int s = 0;
                    for (int j = lg; j < qlen; j += G) s += smat[st[j] * 5 + sq[j]];
                    for (int o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o);
                    score = s;
                } else {
                    w = g2a_band(qlen, tlen, smat[0], P.o_del, P.e_del, P.o_ins, P.e_ins, w2);
                    row_bytes = g2a_row_bytes(qlen, w);
                    const uint64_t need = (uint64_t)row_bytes * tlen;
                    uint8_t* zw = zl;
                    if (fixed + need > (uint64_t)B) {
                        if (!BIG) {
                            status = G2A_DEFERRED;
                            break;
                        }
                        if (need > P.scratch_stride) {
                            status = G2A_BADTRACE;
                            break;
                        }
                        zw = P.scratch + (uint64_t)blockIdx.x * P.scratch_stride;
                    }
                    dp = true;
                    score = global_dp<G>(lane, qlen, tlen, w, sq, st, eh, zw, row_bytes, smat, P.o_del, P.e_del,
                                         P.o_ins, P.e_ins);
                    if (BIG && zw != zl) __threadfence();  // the first lane reads what the others stored
                    z = zw;
                }
                if (score == last_sc) break;
                last_sc = score;
                w2 <<= 1;
                if (!(++i < 3 && score < T.truesc - P.a)) break;
            }
        }
        group_fence();
        if (lg == 0) finish_region(P, T, status, score, tries, dp, w, row_bytes, rev, fb, eh, sq, st, z);
    }
}

// What the host loop of smem_reg2aln did per region, one lane per record: the record's read
// (by bisection over rec_off, as fin_write_kernel finds it), the statuses that need no
// alignment, the test at the head of bwa_fix_xref2 (software/bwa.c:195-199) when a contig
// table is resident, else the task, its first band's shape and its lane-group class.  The
// lists are filled a wave at a time: ballot, rank among the wave's lanes of the class, one
// atomic per wave and class.
__global__ __launch_bounds__(64) void g2a_prep_kernel(G2aPrepParams P) {
    const uint32_t k = blockIdx.x * 64u + threadIdx.x;
    const int lane = (int)threadIdx.x;
    int cls = -1;  // 0..2: 16 / 32 / 64 lanes, 3: scratch tier; -1: settled here
    uint64_t big_need = 0;
    if (k < P.n_rec) {
        uint32_t lo = 0, hi = P.n_reads;  // the last r with rec_off[r] <= k
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (P.rec_off[mid] <= (uint64_t)k) lo = mid;
            else hi = mid;
        }
        const uint32_t r = lo;
        Aln A;
        A.pos = -1, A.is_rev = 0, A.n_cigar = 0, A.NM = 0, A.score = 0, A.tries = 0, A.status = G2A_OK;
        A.cigar_off = 0, A.md_off = 0, A.md_len = 0, A.pad = 0;
        uint64_t ri = k;
        bool have = true;
        if (P.idx) {
            ri = P.idx[k];
            if (P.reg_range && (ri < P.reg_range[r] || ri >= P.reg_range[r + 1])) {
                have = false;  // the call is refused (SMEM_E_ARG): nothing is read through this index
                atomicAdd(&P.cnt[G2A_N_BADIDX], 1u);
                A.status = G2A_UNMAPPED;
            }
        }
        if (have) {
            const G2aReg* R = P.regs + ri;
            const int64_t rb = R->rb, re = R->re;
            const int qb = R->qb, qe = R->qe;
            const int64_t l_query = (int64_t)(P.offs[r + 1] - P.offs[r]);
            if (rb < 0 || re < 0) {  // software/bwamem.c:1489
                A.status = G2A_UNMAPPED;
            } else if (qb < 0 || (int64_t)qe > l_query) {  // (the host-buffer call refuses these before the launch)
                A.status = G2A_BADTRACE;
                atomicAdd(&P.cnt[G2A_N_BADTRACE], 1u);
            } else if (qe <= qb || rb >= re || (rb < P.l_pac && re > P.l_pac) || re > 2 * P.l_pac) {
                A.status = G2A_NOCIGAR, A.NM = -1, A.tries = 1;  // bwa_gen_cigar2 returns 0 (software/bwa.c:106-108)
            } else {
                bool xref = false;
                if (P.ctg.off) {
                    // the head of bwa_fix_xref2: the contig of the region's middle on the forward
                    // strand, its ends on the mapping strand
                    const int64_t m = (rb + re) >> 1;
                    const bool rev = m >= P.l_pac;
                    const int64_t fm = rev ? (P.l_pac << 1) - 1 - m : m;  // bns_depos
                    const int id = g2a_pos2rid(P.ctg.off, P.ctg.n, P.l_pac, fm);
                    if (id >= 0) {
                        const int64_t off = P.ctg.off[id], len = P.ctg.len[id];
                        const int64_t cb = rev ? (P.l_pac << 1) - (off + len) : off, ce = cb + len;
                        xref = cb > rb || ce < re;
                    }
                }
                if (xref) {
                    A.status = G2A_XREF;
                    atomicAdd(&P.cnt[G2A_N_XREF], 1u);
                } else if (qe - qb > G2A_MAX_QLEN || re - rb > (int64_t)G2A_MAX_TLEN) {
                    A.status = G2A_REJECT;
                } else {
                    G2aTask T;
                    T.q_off = P.offs[r] + (uint64_t)qb, T.rb = rb, T.re = re, T.qlen = qe - qb, T.qb = qb;
                    T.l_query = (int32_t)l_query, T.truesc = R->truesc, T.w = R->w, T.out = k;
                    const int tlen = (int)(re - rb);
                    const int w2 = g2a_first_w2(T.qlen, tlen, T.truesc, P.a, P.o_del, P.e_del, P.o_ins, P.e_ins, P.w, T.w);
                    int n_col = 1;
                    uint64_t need = (uint64_t)g2a_fixed_bytes(T.qlen, tlen);
                    if (!(T.qlen == tlen && w2 == 0)) {
                        const int w = g2a_band(T.qlen, tlen, P.a0, P.o_del, P.e_del, P.o_ins, P.e_ins, w2);
                        n_col = T.qlen < 2 * w + 1 ? T.qlen : 2 * w + 1;
                        need += (uint64_t)g2a_row_bytes(T.qlen, w) * (uint64_t)tlen;
                    }
                    cls = n_col <= 16 ? 0 : n_col <= 32 ? 1 : 2;
                    while (cls < 3 && need > (uint64_t)g2a_group_lds(16 << cls)) ++cls;
                    if (cls == 3) big_need = g2a_scratch_need(T.qlen, tlen, P.a0, P.o_del, P.e_del, P.o_ins, P.e_ins);
                    P.task[k] = T;
                }
            }
        }
        // (a record with a task gets its alignment from the DP kernels)
        if (cls < 0) P.alns[k] = A;
        if (P.rid) P.rid[k] = -1;
    }
    const uint64_t below = (1ull << lane) - 1;
    for (int c = 0; c < 4; ++c) {
        const uint64_t m = __ballot(cls == c);
        if (!m) continue;
        uint32_t base = 0;
        if (lane == __builtin_ctzll(m))
            base = atomicAdd(&P.cnt[c == 3 ? G2A_N_BIG : G2A_N_LIST0 + c], (uint32_t)__builtin_popcountll(m));
        base = __shfl(base, __builtin_ctzll(m));
        if (cls == c) P.list[(uint64_t)c * P.n_rec + base + (uint32_t)__builtin_popcountll(m & below)] = k;
    }
    if (big_need) atomicMax(&P.cur[3], (unsigned long long)big_need);
}

}  // namespace
}  // namespace smem

extern "C" hipError_t smem_launch_g2a_prep(const smem::G2aPrepParams* P, hipStream_t st) {
    if (P->n_rec == 0) return hipSuccess;
    hipLaunchKernelGGL(smem::g2a_prep_kernel, dim3((P->n_rec + 63u) / 64u), dim3(64), 0, st, *P);
    return hipGetLastError();
}

extern "C" hipError_t smem_launch_g2a(const smem::G2aParams* P, int group, hipStream_t st) {
    using namespace smem;
    if (P->n == 0) return hipSuccess;
    const uint32_t per = 64u / (uint32_t)group, want = (P->n + per - 1) / per;
    const uint32_t grid = want < (uint32_t)G2A_GRID_MAX ? want : (uint32_t)G2A_GRID_MAX;
    const dim3 g(grid), b(64);
    if (group == 16) hipLaunchKernelGGL((g2a_kernel<16, 4 * g2a_group_lds(16), false>), g, b, 0, st, *P);
    else if (group == 32) hipLaunchKernelGGL((g2a_kernel<32, 2 * g2a_group_lds(32), false>), g, b, 0, st, *P);
    else if (group == 64) hipLaunchKernelGGL((g2a_kernel<64, g2a_group_lds(64), false>), g, b, 0, st, *P);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

extern "C" hipError_t smem_launch_g2a_big(const smem::G2aParams* P, uint32_t blocks, hipStream_t st) {
    using namespace smem;
    if (P->n == 0 || blocks == 0) return hipSuccess;
    const uint32_t grid = P->n < blocks ? P->n : blocks;
    hipLaunchKernelGGL((g2a_kernel<64, G2A_LDS_BIG, true>), dim3(grid), dim3(64), 0, st, *P);
    return hipGetLastError();
}
