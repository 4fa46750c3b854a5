// smem_kernels.hip — CDNA4 (gfx950) kernels of the SMEM seeding engine.
//
// seed_kernel runs, per read, the whole seeding loop BWA-MEM runs on the CPU
// (software/bwamem.c:453-460 -> smem_next2 :244-305 -> bwt_smem1
// software/bwt.c:776-835 -> bwt_extend :416-429 -> bwt_2occ4/bwt_occ4
// :207-215/:187-204), bit-exact, with no host round trip per iteration.
//
// Execution model:
//  * persistent grid, one read per lane; a lane that finishes pulls the next
//    read from a global work counter, so the grid drains when every read is
//    taken (every lane reaches the exit test each time it is idle);
//  * each lane is a state machine whose every transition path ends in exactly
//    one bwt_extend, so all live lanes of a wave issue their Occ-bucket loads
//    from the same instruction each iteration (one reconvergence point per
//    extend instead of four nested loops diverging);
//  * the FM index stays resident in HBM in the reference's interleaved layout
//    (64-B bucket = 4 x u64 checkpoint + 8 x u32 of 2-bit symbols per 128
//    BWT symbols, software/bwt.h:72-73); rank inside a bucket is computed
//    with bit-plane popcounts (v_bcnt) instead of the 1 KB byte LUT;
//  * Occ buckets are fetched cooperatively by LDS-DMA: every wave-instruction
//    moves 16 whole 64-B buckets (4 lanes x 16 B) into the wave's LDS image;
//  * the forward / prev / curr lists live in a per-lane scratch arena as
//    16-B packed entries, prev[j+1] prefetched while prev[j] is extended;
//  * matches are appended to the read's output region as bwt_smem1 emits
//    them; reversing and merging (software/bwt.c:830, software/bwamem.c:280-301)
//    happen in finalize_kernel, off the latency-bound loop.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include "smem_kernels.h"
#include "occ_rank.h"

namespace smem {

// ---- packed list entries (forward / prev / curr lists): 16 B instead of 32 B.
// x0, x1, x2 < 2^34 (seq_len checked on the host), query end < 2^26.
struct PIntv {
    uint32_t x0, x1, x2, hi;  // hi = x0>>32 | x1>>32 << 2 | x2>>32 << 4 | end << 6
};

__host__ __device__ __forceinline__ uint4 pack_p(uint64_t x0, uint64_t x1, uint64_t x2, uint32_t end) {
    return make_uint4((uint32_t)x0, (uint32_t)x1, (uint32_t)x2,
                      (uint32_t)(x0 >> 32) | (uint32_t)(x1 >> 32) << 2 | (uint32_t)(x2 >> 32) << 4 | end << 6);
}

__device__ __forceinline__ uint64_t p_x0(const uint4& v) { return (uint64_t)(v.w & 3) << 32 | v.x; }
__device__ __forceinline__ uint64_t p_x1(const uint4& v) { return (uint64_t)((v.w >> 2) & 3) << 32 | v.y; }
__device__ __forceinline__ uint64_t p_x2(const uint4& v) { return (uint64_t)((v.w >> 4) & 3) << 32 | v.z; }
__device__ __forceinline__ uint32_t p_end(const uint4& v) { return v.w >> 6; }

// ---- query bases through a 16-byte window held in registers; the window
// is loaded in the uniform section (the state machine yields until it is)
template <bool BSEL = false>
__device__ __forceinline__ int qsel(uint32_t o0, int i, const uint4& qv) {
    const uint32_t a = o0 + (uint32_t)i;  // batches hold < 2^32 bases
    if constexpr (BSEL) {  // the window's half by one bit test, the byte by a 64-bit shift
        const uint64_t h0 = (uint64_t)qv.y << 32 | qv.x, h1 = (uint64_t)qv.w << 32 | qv.z;
        return (int)(((a & 8) ? h1 : h0) >> ((a & 7) * 8) & 0xff);
    }
    uint32_t w;
    {
        const uint32_t sel = (a >> 2) & 3;
        w = sel == 0 ? qv.x : (sel == 1 ? qv.y : (sel == 2 ? qv.z : qv.w));
    }
    return (int)((w >> ((a & 3) * 8)) & 0xff);
}

// the 16 bases of a query window as 2-bit codes, the first base highest (4 bytes b0..b3 of a word times
// 2^30 + 2^20 + 2^10 + 1 leave b0 << 6 | b1 << 4 | b2 << 2 | b3 in the top byte; the other partial products
// fall on bits of their own below it), and the mask of its ambiguous bases (byte > 3), bit j = base j
__device__ __forceinline__ uint32_t win_codes(const uint4& qv) {
    auto c = [](uint32_t w) { return ((w & 0x03030303u) * 0x40100401u) >> 24; };
    return c(qv.x) << 24 | c(qv.y) << 16 | c(qv.z) << 8 | c(qv.w);
}
__device__ __forceinline__ uint32_t win_ambig(const uint4& qv) {
    auto n = [](uint32_t w) {
        const uint32_t t = w & 0xFCFCFCFCu;
        const uint32_t y = (((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t) & 0x80808080u;  // bit 7 of every byte that is not 0
        return ((y >> 7) * 0x01020408u) >> 24;
    };
    return n(qv.x) | n(qv.y) << 4 | n(qv.z) << 8 | n(qv.w) << 12;
}

enum Phase : int {
    P_BWD_RES = 0,  // consume a backward extend        (software/bwt.c:815-825)
    P_BWD_J,        // next prev[j] / end of a step      (software/bwt.c:812, 827-828)
    P_FWD_RES,      // consume a forward extend          (software/bwt.c:795-799)
    P_FWD,          // next forward position             (software/bwt.c:791-803)
    P_FWD_DONE,     // reverse + ret                     (software/bwt.c:805-808)
    P_BWD_STEP,     // start backward position i         (software/bwt.c:810-812)
    P_SMEM_END,     // end of one bwt_smem1              (software/bwamem.c:261-278)
    P_OVF,          // output capacity exceeded: hand the read to the overflow pass
    P_NEXT2,        // start of one smem_next2 call      (software/bwamem.c:247-258)
    P_SMEM_BEGIN,   // start of one bwt_smem1            (software/bwt.c:782-789)
    P_FETCH,        // next read from the work counter
    P_BWD_WAIT,     // seed_wp_kernel: the wave is extending the step's entries
    P_BWD_DONE,     // seed_wp_kernel: every entry of the step extended
    P_KSCAN,        // seed_wp_kernel SKIP: collect the call's first bases for the start probe
    P_KRES,         // seed_wp_kernel SKIP: consume the start probe (the forward string of d bases)
    P_KEND,         // seed_wp_kernel SKIP: consume the probe of the longest virtual entry at a call's end
    P_EXIT
};

// bucket b's 16-B chunk as scalar base + 32-bit byte offset (the host keeps
// the index below 4 GiB), so the DMA takes the saddr form
__device__ __forceinline__ const uint32_t* boff(const uint32_t* __restrict__ bwt, uint32_t b, uint32_t chunk) {
    return reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(bwt) + (b * 64u + chunk * 4u));
}

#define LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))

// ---- Occ192: 64-B lines of 192 BWT symbols (a third fewer index bytes than
// Occ64, and more k / l pairs in one line).  Chunk 0: Occ(C), Occ(G), Occ(T)
// before the line's second 64-symbol block (34 bits: low 32 in words 0-2,
// bits 32-33 in word 3 bits 0-5) and the C / G / T counts of that block
// (7 bits each, word 3 bits 6-26).  Chunks 1-3: the line's three blocks of
// 64 symbols, as Occ64's symbol words.  A rank in block r of a line reads
// chunk 0 and chunk 1 + r (still two 16-B loads): r = 0 subtracts the
// block's symbols after the position, r = 1 adds those up to it, r = 2 adds
// the middle block's counts as well.  Slot tags stay the 64-symbol block.
__device__ __forceinline__ void rank192(const Bucket32& v, uint64_t kk, uint64_t& tC, uint64_t& tG, uint64_t& tT) {
    const uint32_t b = (uint32_t)(kk >> 6), r = b - 3u * (b / 3u), p = (uint32_t)(kk & 63);
    uint32_t C, G, T;
    count_cgt4(v.sym, p, C, G, T);
    const uint64_t c0 = occ_cgt(v.cnt, 0), g0 = occ_cgt(v.cnt, 1), t0 = occ_cgt(v.cnt, 2);
    if (r == 0) {
        uint32_t C6, G6, T6;
        count_cgt4(v.sym, 63, C6, G6, T6);
        tC = c0 - (C6 - C);
        tG = g0 - (G6 - G);
        tT = t0 - (T6 - T);
    } else {
        const uint32_t w = r == 2 ? v.cnt.w : 0u;
        tC = c0 + ((w >> 6) & 127u) + C;
        tG = g0 + ((w >> 13) & 127u) + G;
        tT = t0 + ((w >> 20) & 127u) + T;
    }
}

// extend_counts64 (occ_rank.h) on Occ192 lines
template <bool BSEL = false>
__device__ __forceinline__ void extend_counts192(uint64_t primary, const uint64_t* L2, uint64_t a, uint64_t b, uint64_t s,
                                                 int c, uint64_t kk, uint64_t ll, const Bucket32& vk, const Bucket32& vl,
                                                 uint64_t& na, uint64_t& nb, uint64_t& ns) {
    uint64_t tk1, tk2, tk3, tl1, tl2, tl3;
    rank192(vk, kk, tk1, tk2, tk3);
    rank192(vl, ll, tl1, tl2, tl3);
    extend_from_occ<BSEL>(primary, L2, a, b, s, c, kk, ll, tk1, tk2, tk3, tl1, tl2, tl3, na, nb, ns);
}

// the two 16-B chunks of 64-symbol block b: Occ64 bucket b, or Occ192 line b / 3
template <bool L192>
__device__ __forceinline__ void block_chunks(const uint32_t* __restrict__ occ, uint32_t b, const uint32_t*& c0,
                                             const uint32_t*& c1) {
    if constexpr (L192) {
        const uint32_t line = b / 3u;
        c0 = boff(occ, line, 0);
        c1 = boff(occ, line, 4u * (1u + b - 3u * line));
    } else {
        c0 = boff(occ, b >> 1, (b & 1) * 8);
        c1 = boff(occ, b >> 1, (b & 1) * 8 + 4);
    }
}

// offsets of work item `it` (read_ids maps overflow-pass items to reads)
__device__ __forceinline__ void next_offsets(const SeedParams& P, int it, uint32_t& o0, int& len, int& rid) {
    if (it >= P.n_items) {
        len = 0;
        return;
    }
    rid = P.read_ids ? P.read_ids[it] : it;
    const uint64_t a = P.offs[rid], b = P.offs[rid + 1];
    o0 = (uint32_t)a;
    len = (int)(b - a);
}

// chip-wide 100 MHz clock: wave start / end times comparable across XCDs
__device__ __forceinline__ uint64_t rtstamp() {
    uint64_t t;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}

// ======================================================================
// seed_wp_kernel: the same loop with the backward phase wave-parallel over
// list entries (variants 40-43).
//
// A backward step at position i extends every interval of `prev` with the
// same base q[i], and the extends are independent (software/bwt.c:812-826).
// prev is nested (prev[0] is the longest match, each entry's SA interval
// contains the one before it), so the extended sizes are non-decreasing in
// the entry index: the entries that fail (size < min_intv) are a prefix,
// only entry 0 can become a SMEM (the fail branch needs curr->n == 0 and, for
// a second failure, mem's last start is already i + 1), and the survivors
// keep the first of each run of equal sizes (:823).  So a step is one ballot
// of "survives", one of "kept", and a prefix rank of the kept entries -- no
// entry depends on another's result.
//
// Lanes 0 .. OWN-1 of a wave own reads (the smem_next2 / bwt_smem1 state
// machine, as seed_kernel's lanes); every lane of the wave executes one
// bwt_extend per iteration:
//  * an owner in a forward extension (software/bwt.c:791-805: a serial chain)
//    extends its own interval;
//  * every other lane (owners waiting on a backward step, lanes >= OWN, idle
//    owners) takes the next entry of some owner's backward step: the owners'
//    remaining entry counts are prefix-summed across the wave (DPP), owner o
//    gets the free lanes of ranks [excl_o, excl_o + take_o), and each worker
//    finds its owner from the start marks (one LDS scatter + one ballot);
//  * the worker extends the entry, and the kept results are written straight
//    into the owner's curr list (in place over prev: curr[k] is written after
//    prev[>= k] was read, software/bwt.c:828) at the rank the kept ballot gives.
// An owner's step therefore takes one iteration when enough lanes are free,
// instead of one per entry, and the per-entry advance (seed_kernel's
// BWD_RES block) is gone; the lists live in LDS (NL entries per owner, OWN
// owners per wave: twice seed_kernel's entries per list in the same LDS),
// entries beyond NL in the owner's arena.
// ======================================================================
template <int OWN, int NL, bool PAIR, bool DPOS = false>
struct WpWave {
    uint4 e[NL][OWN];     // owners' lists: index k < NL at slot (lr - k) mod NL
    // step descriptors, by owner lane (DPOS: by the task position where the owner's entries start):
    // j, curr_n, prev_off, c | lr << 2 | last_x2 bits 32-33 << 8 | i << 10; min_intv, last_x2 low word,
    // prev_n (DPOS: the owner lane; SKIP: | dp << 24), kc
    uint4 d0[DPOS ? 64 : OWN];
    uint4 d1[DPOS ? 64 : OWN];
    uint4 q[OWN];         // query windows (LDS-DMA landing slots)
    uint4 noff[OWN];      // the next read's offs[rid], offs[rid + 1] (LDS-DMA landing slots)
    uint64_t res[DPOS ? 1 : 64];  // extend result sizes by lane (PAIR: of the lane's last entry; DPOS: in d1,
                                  // which the workers have read before the results are written)
    uint64_t res1[PAIR ? 64 : 1];  // PAIR: of the lane's first entry
    uint8_t tabS[64];     // owner whose segment starts at task position p (0xFF: none)
    uint8_t tabP[64];     // free-lane rank -> lane
    uint4 pend[2][OWN];   // each owner's even-indexed raw record, held for the odd one that completes its line
};

// the OR of v over the 64 lanes (the same pattern; lane 63 holds it)
__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);  // row_shr:2
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);  // row_shr:4
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);  // row_shr:8
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// inclusive prefix sum over the 64 lanes (the row_shr / row_bcast pattern of
// ksw_device.h's scan_max)
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);  // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);  // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);  // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31
    return v;
}

// set bits of m below this lane
__device__ __forceinline__ uint32_t mbcnt64(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__device__ __forceinline__ int hibit64(uint64_t m) { return 63 - __builtin_clzll(m); }

// A register that no instruction sets: the value is whatever the lane's register held.  Defined
// (an empty asm "writes" it), unlike an uninitialised variable, and arbitrary: only for a variable
// that every lane which goes on to use it assigns first (seed_wp_kernel's DIET 16)
__device__ __forceinline__ uint32_t idle_u32() {
    uint32_t v;
    asm volatile("" : "=v"(v));
    return v;
}

// A lane flag the compiler cannot trace back to the compares it came from (a v_cndmask and a v_cmp).
// seed_wp_kernel SKIP: with fwdreq left as three compares of `phase`, every select by it below
// (ra / rb / rs, the probe's sides) compiled to a branch tree over the phase's ranges, walked whole
// by every wave-iteration (DESIGN.md §5 "The skipping arm's fixed cost")
__device__ __forceinline__ bool lane_flag(bool b) {
    uint32_t v = b ? 1u : 0u;
    asm volatile("" : "+v"(v));
    return v != 0u;
}

// seed_wp_kernel SKIP: the k-mer table's slot of a string of lq bases, its codes the low bits of `codes`
// (top: the highest of K bases' worth).  Level lq starts at (4^lq - 4) / 3 = 0b0101..01 (lq ones) - 1;
// lq is clipped to the table's levels (only a broken state is: the probe stays in the table)
__device__ __forceinline__ uint32_t kt_slot(uint32_t codes, int lq, int K, bool top) {
    lq = lq < 1 ? 1 : (lq > K ? K : lq);
    const uint32_t code = (top ? codes >> (2 * (K - lq)) : codes) & ((1u << (2 * lq)) - 1u);
    return (0x55555555u >> (32 - 2 * lq)) - 1u + code;
}

// LDS accesses of one wave execute in order; this keeps the compiler from
// moving them across the point where another lane's write must be seen
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

// PAIR: a worker lane takes two consecutive entries of a step (two extends
// in flight per lane: twice the requests per wave-iteration)
// KT: an extend whose result is a string of at most P.kt_k bases reads that
// string's bi-interval from the k-mer table (one 16-B probe; the table of
// k = 11 is 90 MB and stays in the 256 MB MALL) instead of two Occ buckets
// and the rank: a bi-interval is a function of the string alone, so the
// result is bwt_extend's.  Owners keep the codes of their forward string's
// first k bases and of the k bases from the backward position (variant 23's
// bookkeeping); the step descriptor carries the latter and the position.
// DPOS: the segment starts' mask by a DPP OR over the owners and each owner's
// descriptor stored at its start position, so a worker reads its owner's
// descriptor one LDS round after the scan (three rounds before the loads:
// start marks, owner, descriptor, entry -> descriptor, entry)
// OPT (A/B of the memory-issue order; default all): 1 claim the next read when the current one ends
// (else as soon as it starts), 2 arena entries in a wave-uniform branch with their own wait (else
// inline: the join's wait then runs every iteration and covers the owners' result-store acks), 4 the
// query-window / offsets DMA and the claim issued after the entry has landed (else before it: the
// compiler's wait for the entry covers them), 8 the claim as one hand-issued atomic per wave waited
// for by the iteration's vmcnt(0) (else the compiler's atomicAdd at the top, which waits for it)
// DIET (A/B of the instructions one wave-iteration issues, DESIGN.md §5 "The iteration's instruction
// diet"; every arm is in unless its bit is set in OPT, so the default stays OPT = 15): 16 the uniform
// section's temporaries start undefined in lanes without a task (out: zeroed, a v_mov each, every
// iteration, for values nothing reads), 32 no `out` flag (a lane is at P_FWD_RES at the end of a pass
// exactly when P_FWD has just asked for the extend), 64 the selects by base as two bit tests (sel4b;
// out: sel4's compare chain, which compiles to a branch tree), 128 the query byte by one bit test and
// a 64-bit shift (out: qsel's compare chain, a branch tree again)
// SKIP (with KT; DESIGN.md §5 "Virtual short entries"): the entries of a call whose strings are shorter
// than dp bases are not stored and not extended.  With D the largest level up to the table's depth at
// which every string of D + 1 bases occurs (level depth + 1 is not stored: the build reduces it on the
// fly, kmer_next_level_min_kernel) and minsz[L] the smallest interval size of level L, dp is a
// level <= D with minsz[dp] >= min_intv: the host passes one for a read's first calls (P.kt_dp0) and one
// for its re-seeding calls (P.kt_dp1; smem_gpu.cpp fill_params).  Up to dp bases every forward extend
// changes the size and none falls below min_intv, so a call starts with one probe of its first
// d = min(dp, bases before an ambiguous one or the read's end) bases and counts the d - 1 shorter
// forward entries as virtual (nv: the forward lengths 1..nv).  In a backward step a virtual entry whose
// string stays below dp bases survives and is never a duplicate (the entry kept before it is a proper
// right extension, strictly smaller), so it gets no task; the one whose string reaches exactly dp bases
// is probed (the step's last task, after the real entries) and is real from then on.  A call that ends
// (i == -1 or an ambiguous base) with only virtual entries left probes the longest at its length for
// the record.  dp < 2: the call runs the plain path.  (No loops over bases or levels in the owners'
// blocks, and no further WP_EMIT site: the first version had them and doubled the launch's SALU)
// (the body of both kernels below: seed_wp_kernel keeps its eight parameters and its symbol)
// WIDE (SKIP only; the other arms are always wide): the extend's counts in 64 bits (extend_counts64), for an
// index in which a base occurs 2^32 times or more; else in 32 (extend_counts32; the host's rule is
// smem_occ_narrow_ok)
template <int OWN, int NL, int PRIO, int WPE, bool PAIR, bool KT, bool DPOS, int OPT, bool SKIP, bool WIDE = true>
__device__ __forceinline__ void seed_wp_body(const SeedParams& P) {
    constexpr int DIET = ~OPT;  // bits 16-128 of OPT take an arm of the diet out
    static_assert(!SKIP || (KT && !PAIR && !DPOS), "SKIP probes the k-mer table and keeps prev_n | dp << 24 in the descriptor");
    static_assert(!(DPOS && PAIR), "DPOS keeps the owner lane where PAIR keeps prev_n");
    constexpr uint32_t PR = PAIR ? 2u : 1u;  // entries per worker lane
    const int K = KT && P.kt ? P.kt_k : 0;
    // SKIP: the probe depth of a read's first calls (min_intv = start_width) and of its re-seeding calls
    // (min_intv <= split_width + 1), chosen on the host (smem_kmer_probe_depth); at most the table's depth K
    // (dp == K: the table's deepest level is probed, and kc, which holds K bases, is read whole)
    const uint32_t DP0 = SKIP && K > 0 && P.kt_dp0 <= K ? (uint32_t)P.kt_dp0 : 0u;
    const uint32_t DP1 = SKIP && K > 0 && P.kt_dp1 <= K ? (uint32_t)P.kt_dp1 : 0u;
    static_assert(OWN >= 1 && OWN <= 64 && NL >= 2 && NL < 32, "owners per wave / list entries");
    __shared__ WpWave<OWN, NL, PAIR, DPOS> wlds[4];
    WpWave<OWN, NL, PAIR, DPOS>* L = &wlds[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
    uint64_t* const RES = DPOS ? reinterpret_cast<uint64_t*>(&L->d1[0]) : &L->res[0];
    const int me = (int)(threadIdx.x & 63);
    const uint64_t wave_g = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u);  // lane 0's global index
    const uint32_t cap = P.cap_list;
    // an owner's arena: [0, cap) the forward list beyond the ring, [cap, 2 cap) curr / prev beyond NL;
    // one per owner (OWN a wave, numbered from wown), not per lane: the batch's scratch is 64 / OWN
    // times smaller (smem_gpu.cpp seed_arenas)
    const uint64_t wown = (wave_g >> 6) * (uint64_t)OWN;
    PIntv* __restrict__ bp = reinterpret_cast<PIntv*>(P.scratch + (wown + (uint64_t)(me < OWN ? me : 0)) * 2ull * cap);

    int phase = me < OWN ? P_FETCH : P_EXIT;  // lanes >= OWN only execute extends
    int item = -1, len = 0;
    // next read: -2 nothing claimed, -5 claim in flight, -1 claimed, -3 its offsets to be fetched, -4 in
    // flight, >= 0 loaded.  Claimed when the current read ends (OPT 1; claimed when it starts, a read
    // held in reserve behind a busy owner lengthened the launch's tail).  The claim's atomic (OPT 8)
    // and the offsets' LDS-DMA are waited for by the iteration's vmcnt(0), never on their own: a wave
    // stalled a memory round trip per read for each before (the compiler's atomicAdd waits for the
    // result to broadcast it)
    int nitem = 0, nlen = -2;
    uint32_t clead = 0;  // the last claim's leader lane (wave-uniform); its atomic's return lands in no0
    int rid = 0, nrid = 0;
    uint32_t o0 = 0, no0 = 0;
    uint32_t qb = ~0u, qwant = ~0u;
    uint4 qv = {0, 0, 0, 0};
    uint32_t raw_n = 0, calls_n = 0;
    int start = 0, ori_start = 0;
    int x = 0, min_intv = 1, middle = 0, i = 0, cur_c = 0;
    uint32_t j = 0;
    uint32_t kc = 0;  // KT: forward, the string's codes; backward, the K bases from position i (one register: never both)
    uint32_t nv = 0;  // SKIP: virtual entries left (forward lengths 1..nv)
    uint64_t ik0 = 0, ik1 = 0, ik2 = 0;
    uint32_t ikend = 0;  // ik's end; from the end of the forward phase on, bwt_smem1's return value
    // fwd_n is prev_off as well: forward, the entries pushed; backward, where prev[NL ..] sits in the arena
    uint32_t fwd_n = 0, prev_n = 0, curr_n = 0;
    uint32_t lr = 0;           // forward: the ring position; backward: the slot of list index 0
    uint32_t fail0 = 0;        // bit 0: entry 0 of the current step failed (its SMEM candidate); SKIP, bit 1: the step has a probe (WP_VP)
    uint64_t last_x2 = 0;      // size of the last entry kept in curr (dedup across chunks of a step)
    uint32_t mem_last_start = ~0u;  // the start of the call's last record (~0: none yet, mem->n == 0)
    uint32_t max_len = 0, max_x2 = 0, max_mid = 0;
    uint4 head = {0, 0, 0, 0};  // prev[0] of the current step
    uint64_t na = 0, nb = 0, ns = 0;  // an extend's result (SKIP: before its own probe, an owner's na holds the table slot)
    if (P.tspan && me == 0) atomicMax(reinterpret_cast<unsigned long long*>(P.tspan), ~(unsigned long long)rtstamp());

#define QBLK(pos) ((o0 + (uint32_t)(pos)) & ~15u)
#define WSLOT(r_, k_) ((r_) >= (k_) ? (r_) - (k_) : (r_) + (uint32_t)NL - (k_))
// a SMEM of the current call: the raw log entry, the merge's keep count and
// the longest match (software/bwt.c:817-819, software/bwamem.c:266-270, 284-292)
// Only what the merge keeps is logged (every match; a sub-match of at least
// half the longest match that ends after the call's start), tagged with the
// call's ordinal and the sub-match bit (smem_kernels.h), so the read's logged
// count is its final interval count.  Records go out as whole 64-B lines: an
// even-indexed one waits in LDS for the odd one that follows it.
#define WP_EMIT(e_)                                                                                          \
    {                                                                                                        \
        const uint4 me_ = (e_);                                                                              \
        const uint32_t b_ = (uint32_t)(i + 1), en_ = p_end(me_);                                             \
        if (!middle || (en_ - b_ >= (max_len >> 1) && en_ > (uint32_t)ori_start)) {                          \
            if (raw_n >= P.cap_intv) {                                                                       \
                phase = P_OVF;                                                                               \
            } else {                                                                                         \
                const uint64_t x0_ = p_x0(me_), x1_ = p_x1(me_), x2_ = p_x2(me_);                            \
                const uint32_t tag_ = (uint32_t)(x0_ >> 32) | calls_n << (RAW_ORD_SHIFT - 32) |              \
                                      (middle ? RAW_SUB_BIT << (RAW_ORD_SHIFT - 32) : 0u);                   \
                const uint4 lo_ = make_uint4((uint32_t)x0_, tag_, (uint32_t)x1_, (uint32_t)(x1_ >> 32));     \
                const uint4 hi_ = make_uint4((uint32_t)x2_, (uint32_t)(x2_ >> 32), en_, b_);                 \
                if (raw_n & 1) {                                                                             \
                    uint4* ln_ = reinterpret_cast<uint4*>(P.out_intv + (uint64_t)item * P.slot_intv + (raw_n - 1)); \
                    ln_[0] = L->pend[0][me];                                                                 \
                    ln_[1] = L->pend[1][me];                                                                 \
                    ln_[2] = lo_;                                                                            \
                    ln_[3] = hi_;                                                                            \
                } else {                                                                                     \
                    L->pend[0][me] = lo_;                                                                    \
                    L->pend[1][me] = hi_;                                                                    \
                }                                                                                            \
                ++raw_n;                                                                                     \
            }                                                                                                \
        }                                                                                                    \
        mem_last_start = b_;                                                                                 \
        if (!middle && en_ - b_ >= max_len) {                                                                \
            max_len = en_ - b_;                                                                              \
            max_x2 = p_x2(me_) > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)p_x2(me_);                          \
            max_mid = (en_ + b_) >> 1;                                                                       \
        }                                                                                                    \
    }

// the query window for owners that want one, the next read's offsets, and (OPT 8) one returning atomic
// per wave for every owner that wants its next read, issued by hand: not waited for here, read at the
// top of the next iteration after the iteration's vmcnt(0); early clobber, so that the return
// register does not overlap the address.  OPT 4 issues this after the entry has landed and before the
// buckets (all land in one round trip); else before the entry, whose wait then covers them.
#define WP_ISSUE()                                                                                                            \
    {                                                                                                                         \
        if (ld_q) __builtin_amdgcn_global_load_lds(P.codes + qwant, LDS_PTR(&L->q[0]), 16, 0, 0);                             \
        if (nlen == -3) {                                                                                                     \
            __builtin_amdgcn_global_load_lds(P.offs + nrid, LDS_PTR(&L->noff[0]), 16, 0, 0);                                  \
            nlen = -4;                                                                                                        \
        }                                                                                                                     \
        const bool wc_ = nlen == -2 && ((OPT & 1) ? phase == P_FETCH : phase != P_EXIT);                                      \
        const uint64_t want_claim = (OPT & 8) ? __ballot(wc_) : 0ull;                                                         \
        if (want_claim) {                                                                                                     \
            clead = (uint32_t)(__builtin_ffsll((long long)want_claim) - 1);                                                   \
            if (wc_) {                                                                                                        \
                nitem = (int)__popcll(want_claim & ((1ull << me) - 1));                                                       \
                if ((uint32_t)me == clead) {                                                                                  \
                    const int cnt = (int)__popcll(want_claim);                                                                \
                    asm volatile("global_atomic_add %0, %1, %2, off sc0" : "=&v"(no0) : "v"(P.head), "v"(cnt) : "memory");    \
                }                                                                                                             \
                nlen = -5;                                                                                                    \
            }                                                                                                                 \
        }                                                                                                                     \
    }

// the start value of the uniform section's per-task temporaries (see there)
#define WP_IDLE32() ((DIET & 16) ? idle_u32() : 0u)
#define WP_IDLE128() ((DIET & 16) ? make_uint4(idle_u32(), idle_u32(), idle_u32(), idle_u32()) : make_uint4(0, 0, 0, 0))
// the lane yields this pass (DIET 32: nothing to note, see fwdreq)
#define WP_OUT()                         \
    {                                    \
        if constexpr (!(DIET & 32)) out = true; \
    }
// SKIP: this step materialises a virtual entry (the longest one's string reaches dp bases at position i)
#define WP_DP() (middle ? DP1 : DP0)
#define WP_VP() (SKIP && nv != 0 && nv + (uint32_t)(x - i) == WP_DP())
// one forward push (software/bwt.c:797, 802): the ring's oldest entry moves to the arena first
#define WP_PUSH()                                                                                                \
    {                                                                                                            \
        const uint4 fe = pack_p(ik0, ik1, ik2, ikend);                                                           \
        if (fwd_n >= (uint32_t)NL) *reinterpret_cast<uint4*>(bp + cap - 1 - (fwd_n - NL)) = L->e[lr][me];        \
        L->e[lr][me] = fe;                                                                                       \
        lr = lr + 1 == (uint32_t)NL ? 0u : lr + 1;                                                               \
        ++fwd_n;                                                                                                 \
    }

    for (;;) {
        if constexpr (PRIO == 1) __builtin_amdgcn_s_setprio(2);
        if (phase != P_EXIT) {
            if (!(OPT & 8) && nlen == -2 && phase == P_FETCH) {
                nitem = atomicAdd(P.head, 1);  // (the compiler waits for the result here)
                nlen = -1;
            } else {
                if ((OPT & 8) && nlen == -5) {  // the claim returned: the leader's base + this lane's rank
                    nitem += (int)__builtin_amdgcn_readlane(no0, clead);
                    nlen = -1;
                }
                if (nlen == -1) {
                    if (nitem >= P.n_items) {
                        nlen = 0;  // nothing left: the FETCH block exits
                    } else if (P.read_ids) {  // overflow pass: through read_ids (a small launch)
                        next_offsets(P, nitem, no0, nlen, nrid);
                    } else {
                        nrid = nitem;
                        nlen = -3;  // offsets fetched in the uniform section
                    }
                } else if (nlen == -4) {  // landed last iteration
                    const uint4 v = L->noff[me];
                    no0 = v.x;  // batches hold < 2^32 bases: the low words
                    nlen = (int)(v.z - v.x);
                }
            }
        }
        // ---- owners: advance the state machine one pass (seed_kernel's
        // blocks, without the per-entry backward block) ----
        [[maybe_unused]] bool out = false;
        if (phase != P_EXIT) {
            if constexpr (SKIP) {  // the owner's own probe has landed (na: the x[1] side, nb: x[0])
                if (phase == P_KRES) {  // the forward string of i - x bases; the shorter ones stay virtual
                    ik0 = nb; ik1 = na; ik2 = ns;
                    ikend = (uint32_t)i;
                    nv = (uint32_t)(i - x) - 1;
                    phase = P_FWD;
                } else if (phase == P_KEND) {  // the longest virtual entry, now prev[0]: P_BWD_STEP emits it
                    head = pack_p(nb, na, ns, (uint32_t)x + nv);
                    nv = 0;
                    prev_n = 1;
                    phase = P_BWD_STEP;
                }
            }
            if (phase == P_SMEM_END) {
                if (!middle) {  // software/bwamem.c:261-272
                    start = (int)ikend;
                    const int split_len = P.split_len_init < len ? P.split_len_init : len;
                    if (mem_last_start != ~0u && split_len > 0 && (int)max_len >= split_len &&
                        (uint64_t)max_x2 <= (uint64_t)(int64_t)P.split_width) {
                        x = (int)max_mid;  // re-seed from the middle (software/bwamem.c:272-278)
                        min_intv = (int)(max_x2 + 1);
                        middle = 1;
                        phase = P_SMEM_BEGIN;
                    }
                }
                if (phase == P_SMEM_END) {  // the call's records carry its ordinal: nothing else to log
                    ++calls_n;
                    phase = P_NEXT2;
                }
            }
            if (phase == P_OVF) {  // (the record pending in LDS is dropped with the read's log)
                const int slot = atomicAdd(P.ovf_count, 1);
                P.ovf_items[slot] = item;
                phase = P_FETCH;
            }
            if (phase == P_FETCH) {
                if (nlen < 0) {
                    WP_OUT();
                } else if (nitem >= P.n_items) {
                    phase = P_EXIT;
                } else {
                    item = nitem;
                    rid = nrid;
                    o0 = no0;
                    len = nlen;
                    nlen = -2;
                    raw_n = 0;
                    calls_n = 0;
                    start = 0;
                    if (len < P.min_seed_len) {  // mem_chain's guard (software/bwamem.c:600)
                        // (zeros made here, opaque to the compiler: as a constant it hoisted them out of the loop
                        // and, at 128 VGPRs, into a spill slot -- the skipping kernel then 128 VGPRs + 4 spilled
                        // (20 B of scratch a lane) instead of 128 + 0, the plain one 122 VGPRs instead of 118 and no
                        // spill either way; hipcc --cuda-device-only -S, ROCm 7.2.  A compiler that spills here again only costs this
                        // rare path a scratch load: check the .vgpr_spill_count the build reports)
                        uint32_t z;
                        asm volatile("v_mov_b32 %0, 0" : "=v"(z));
                        *reinterpret_cast<uint4*>(P.sizes + 2 * (uint64_t)rid) = make_uint4(z, z, z, z);
                        WP_OUT();
                    } else {
                        phase = P_NEXT2;
                    }
                }
            }
            if (phase == P_NEXT2) {  // software/bwamem.c:247-261
                bool wait_q = false;
                if (start < len && start >= 0) {
                    for (;;) {
                        if (start >= len) break;
                        if (QBLK(start) != qb) { wait_q = true; break; }
                        if (qsel<(DIET & 128) != 0>(o0, start, qv) <= 3) break;
                        ++start;
                    }
                }
                if (wait_q) {
                    qwant = QBLK(start);
                    WP_OUT();
                } else if (start >= len || start < 0) {
                    if (raw_n & 1) {  // an odd count: the last record goes out alone
                        uint4* ln_ = reinterpret_cast<uint4*>(P.out_intv + (uint64_t)item * P.slot_intv + (raw_n - 1));
                        ln_[0] = L->pend[0][me];
                        ln_[1] = L->pend[1][me];
                    }
                    *reinterpret_cast<uint4*>(P.sizes + 2 * (uint64_t)rid) = make_uint4(raw_n, 0, calls_n, 0);
                    phase = P_FETCH;
                } else {
                    ori_start = start;
                    x = ori_start;
                    min_intv = P.start_width;
                    middle = 0;
                    max_len = 0;
                    phase = P_SMEM_BEGIN;
                }
            }
            if (phase == P_SMEM_BEGIN) {  // software/bwt.c:782-789
                if (QBLK(x) != qb) {
                    qwant = QBLK(x);
                    WP_OUT();
                } else {
                    mem_last_start = ~0u;
                    const int qx = qsel<(DIET & 128) != 0>(o0, x, qv);
                    if (qx > 3) {
                        ikend = (uint32_t)(x + 1);
                        phase = P_SMEM_END;
                    } else {
                        if (min_intv < 1) min_intv = 1;
                        const uint64_t lq = (DIET & 64) ? sel4b(qx, P.L2[0], P.L2[1], P.L2[2], P.L2[3])
                                                         : sel4(qx, P.L2[0], P.L2[1], P.L2[2], P.L2[3]);
                        const uint64_t lq1 = (DIET & 64) ? sel4b(qx, P.L2[1], P.L2[2], P.L2[3], P.L2[4])
                                                          : sel4(qx, P.L2[1], P.L2[2], P.L2[3], P.L2[4]);
                        const uint64_t lc = (DIET & 64) ? sel4b(qx, P.L2[3], P.L2[2], P.L2[1], P.L2[0])
                                                         : sel4(qx, P.L2[3], P.L2[2], P.L2[1], P.L2[0]);
                        ik0 = lq + 1;
                        ik2 = lq1 - lq;
                        ik1 = lc + 1;
                        ikend = (uint32_t)(x + 1);
                        if constexpr (KT) kc = (uint32_t)qx;
                        fwd_n = 0;
                        lr = 0;
                        i = x + 1;
                        phase = P_FWD;
                        if constexpr (SKIP) {
                            nv = 0;
                            if (WP_DP() >= 2) phase = P_KSCAN;
                        }
                    }
                }
            }
            if constexpr (SKIP) {
                // the codes of q[x, i) are in kc; the window's bases from i, up to the call's depth, the read's end
                // or an ambiguous base, in one go (no loop: the whole wave would walk it)
                if (phase == P_KSCAN) {
                    bool done = true;
                    if (i < len && (uint32_t)(i - x) < WP_DP()) {
                        done = false;
                        if (QBLK(i) != qb) {
                            qwant = QBLK(i);
                            WP_OUT();
                        } else {
                            const uint32_t off = (o0 + (uint32_t)i) & 15u;
                            const uint32_t rem = min(WP_DP() - (uint32_t)(i - x), (uint32_t)(len - i));
                            const uint32_t inwin = min(rem, 16u - off);
                            const uint32_t nm = win_ambig(qv) >> off;
                            const uint32_t nfree = nm ? (uint32_t)__builtin_ctz(nm) : 16u;  // bases before an ambiguous one
                            const uint32_t take = min(inwin, nfree);
                            if (take) {
                                kc = kc << (2 * take) | (win_codes(qv) << (2 * off)) >> (32 - 2 * take);
                                i += (int)take;
                            }
                            if (take == inwin && inwin < rem) {  // the rest is in the next window
                                qwant = QBLK(i);
                                WP_OUT();
                            } else {
                                done = true;
                            }
                        }
                    }
                    if (done) {
                        if (i - x >= 2) {
                            if (i < len) qwant = QBLK(i);
                            phase = P_KRES;  // -> the probe of q[x, i), on this lane (its slot waits in na)
                            na = kt_slot(kc, i - x, K, false);
                            WP_OUT();
                        } else {
                            phase = P_FWD;
                        }
                    }
                }
            }
            if (phase == P_BWD_DONE) {  // every entry of step i extended (software/bwt.c:815-828)
                if ((fail0 & 1u) && (uint32_t)(i + 1) < mem_last_start) WP_EMIT(head);
                if (phase == P_BWD_DONE) {
                    if (curr_n == 0 && (!SKIP || nv == 0)) {  // software/bwt.c:827 (virtual entries are in curr too)
                        phase = P_SMEM_END;
                    } else {            // :828 swap, next position
                        if constexpr (SKIP) nv -= fail0 >> 1;  // the step's probe made the longest virtual entry real
                        prev_n = curr_n;
                        fwd_n = cap;
                        head = L->e[lr][me];  // curr[0]: index 0 sits in slot lr
                        --i;
                        phase = P_BWD_STEP;
                    }
                }
            }
            if (phase == P_FWD_RES) {  // software/bwt.c:795-799; na = x[1], nb = x[0]
                bool stop = false;
                if (ns != ik2) {
                    WP_PUSH()
                    stop = ns < (uint64_t)min_intv;
                }
                if (stop) {
                    phase = P_FWD_DONE;
                } else {
                    ik0 = nb; ik1 = na; ik2 = ns;
                    ikend = (uint32_t)(i + 1);
                    if constexpr (KT) {
                        if (i + 1 - x <= K) kc = kc << 2 | (uint32_t)(3 - cur_c);  // saturates at the first K bases
                    }
                    ++i;
                    phase = P_FWD;
                }
            }
            if (phase == P_FWD) {  // software/bwt.c:791-803
                bool push = true;
                if (i < len) {
                    if (QBLK(i) != qb) {
                        qwant = QBLK(i);
                        WP_OUT();
                        push = false;
                    } else {
                        const int qi = qsel<(DIET & 128) != 0>(o0, i, qv);
                        if (qi < 4) {
                            cur_c = 3 - qi;
                            if (i + 1 < len) qwant = QBLK(i + 1);
                            phase = P_FWD_RES;  // -> extend (forward), on this lane
                            WP_OUT();
                            push = false;
                        }
                    }
                }
                if (push) {  // ambiguous base, or end of query: push ik and stop
                    WP_PUSH()
                    phase = P_FWD_DONE;
                }
            }
            if (phase == P_FWD_DONE) {  // software/bwt.c:805-808 (the ring read backwards is the reversal)
                head = pack_p(ik0, ik1, ik2, ikend);  // the last push: prev[0]
                if constexpr (KT) {  // the K bases from x (those past the forward string are never read)
                    const uint32_t lf = ikend - (uint32_t)x;
                    if (lf < (uint32_t)K) kc <<= 2 * ((uint32_t)K - lf);
                }
                prev_n = fwd_n;
                fwd_n = cap - fwd_n;
                lr = lr == 0 ? (uint32_t)NL - 1 : lr - 1;  // slot of the last push
                i = x - 1;
                phase = P_BWD_STEP;
            }
            if (phase == P_BWD_STEP) {  // software/bwt.c:810-812
                if (i >= 0 && QBLK(i) != qb) {
                    qwant = QBLK(i);
                    WP_OUT();
                } else {
                    cur_c = i < 0 ? -1 : qsel<(DIET & 128) != 0>(o0, i, qv);
                    if (cur_c > 3) cur_c = -1;
                    if (cur_c >= 0) {
                        j = 0;
                        curr_n = 0;
                        fail0 = WP_VP() ? 2u : 0u;
                        if constexpr (KT) {
                            if (K > 0) kc = (uint32_t)cur_c << (2 * (K - 1)) | kc >> 2;
                        }
                        if (i > 0) qwant = QBLK(i - 1);  // the next step's base
                        phase = P_BWD_WAIT;               // -> the wave extends the step's entries
                        if constexpr (SKIP) {
                            // only virtual entries are left and none reaches dp bases: they all survive, the
                            // step changes nothing (rare: one pass a step)
                            if (prev_n == 0 && !fail0) {
                                --i;
                                phase = P_BWD_STEP;
                                WP_OUT();
                            }
                        }
                    } else {
                        // nothing extends: prev[0] is the only candidate (software/bwt.c:816-819)
                        phase = P_SMEM_END;
                        if ((uint32_t)(i + 1) < mem_last_start) {
                            if (SKIP && prev_n == 0 && nv != 0) {  // prev[0] is virtual: -> its probe, on this lane
                                phase = P_KEND;
                                na = kt_slot(kc, (int)nv + x - i - 1, K, true);
                            } else {
                                WP_EMIT(head);
                            }
                        }
                    }
                }
            }
        }
        // ---- uniform section ----
        if (!__any(phase != P_EXIT)) break;
        // (a lane is at P_FWD_RES here only when P_FWD has just set it: the P_FWD_RES block always leaves it)
        // (the same holds for SKIP's own probes, P_KRES / P_KEND: a lane that extends or probes for itself)
        // (SKIP: both told from the phase once, by a bit test, and kept as lane flags, see lane_flag)
        constexpr uint32_t OWNP_SET = 1u << P_KRES | 1u << P_KEND, FWD_SET = OWNP_SET | 1u << P_FWD_RES;
        const bool ownp = SKIP && lane_flag(((1u << phase) & OWNP_SET) != 0u);
        const bool fwdreq = SKIP ? lane_flag(((DIET & 32) || out) && ((1u << phase) & FWD_SET) != 0u)
                                 : ((DIET & 32) || out) && phase == P_FWD_RES;
        const uint32_t rem = phase == P_BWD_WAIT ? prev_n + (SKIP ? fail0 >> 1 : 0u) - j : 0u;
        const uint32_t slots = (rem + PR - 1) / PR;  // worker lanes the step still needs
        if (!DPOS && rem) {  // what a worker needs of this owner's step
            L->d0[me] = make_uint4(j, curr_n, fwd_n,
                                   (uint32_t)cur_c | lr << 2 | (uint32_t)(last_x2 >> 32) << 8 | (uint32_t)i << 10);
            L->d1[me] = make_uint4((uint32_t)min_intv, (uint32_t)last_x2, SKIP ? prev_n | WP_DP() << 24 : prev_n, kc);
        }
        // the owners' remaining entries laid out in lane order over the free lanes
        const uint32_t incl = wave_scan_add(slots);
        const uint32_t excl = incl - slots;
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        const uint64_t fmask = ~(uint64_t)__ballot(fwdreq);
        const uint32_t nfree = (uint32_t)__popcll(fmask);
        const uint32_t ntask = total < nfree ? total : nfree;
        const uint32_t take = (slots && excl < nfree) ? min(slots, nfree - excl) : 0u;
        const bool freel = (fmask >> me) & 1;
        const uint32_t rank = mbcnt64(fmask);
        uint64_t marks;
        if constexpr (DPOS) {
            if (take) {  // the descriptor where the owner's entries start
                L->d0[excl] = make_uint4(j, curr_n, fwd_n,
                                         (uint32_t)cur_c | lr << 2 | (uint32_t)(last_x2 >> 32) << 8 | (uint32_t)i << 10);
                L->d1[excl] = make_uint4((uint32_t)min_intv, (uint32_t)last_x2, (uint32_t)me, kc);
            }
            if (freel) L->tabP[rank] = (uint8_t)me;
            const uint32_t mlo = wave_or(take && excl < 32 ? 1u << excl : 0u);
            const uint32_t mhi = wave_or(take && excl >= 32 ? 1u << (excl - 32) : 0u);
            marks = (uint64_t)mhi << 32 | mlo;
            wave_lds_fence();
        } else {
            L->tabS[me] = 0xFFu;
            wave_lds_fence();
            if (take) L->tabS[excl] = (uint8_t)me;
            if (freel) L->tabP[rank] = (uint8_t)me;
            wave_lds_fence();
            marks = __ballot(L->tabS[me] != 0xFFu);
        }
        const bool worker = freel && rank < ntask;
        // What only a worker sets and only a worker's results use.  DIET 16 leaves the other lanes'
        // copies ARBITRARY (idle_u32), not zero, so this invariant holds and must keep holding:
        //  * s, o, jj, lro, w0, w1, ent are assigned under `worker` below and read only under `worker`
        //    (surv, keep, rank == s, tabP[s], RES[pp], the stores into the owner's list) or under `far`,
        //    which only a worker sets -- obp, formed from `o` outside the branch, is dereferenced only
        //    there; a forward lane (fwdreq) takes ra / rb / rs / rc from its own state, never from ent / w0,
        //    and the KT path reads w1.w only where !fwdreq, i.e. on a worker (SKIP: a lane that probes for
        //    itself forms a slot from its arbitrary w1 as well and drops it for the one its own block left in
        //    na; kt_slot clips either into the table);
        //  * k0, k1, l0, l1 are loaded under `task` and read under `task` (l0 / l1 only where bl != bk);
        //  * what comes out of arbitrary inputs in a lane without a task (kk, ll, bk, bl) reaches no
        //    address: every load and store below is under `task`, `far`, `keep` or `take`.
        // A new use of any of them outside those conditions reads garbage silently.
        uint32_t s = WP_IDLE32(), o = WP_IDLE32(), jj = WP_IDLE32(), lro = WP_IDLE32();
        bool has2 = false;
        uint4 w0 = WP_IDLE128(), w1 = WP_IDLE128(), ent = WP_IDLE128(), ent2 = {0, 0, 0, 0};
        bool far = false, far2 = false;  // the entry (PAIR: the second) is in the owner's arena
        bool isp = false;                // SKIP: the task is the step's probe (list index prev_n), not an entry
        if (worker) {
            s = (uint32_t)hibit64(marks & ((2ull << rank) - 1ull));  // the segment holding task `rank`
            if constexpr (DPOS) {
                w0 = L->d0[s];
                w1 = L->d1[s];
                o = w1.z;
            } else {
                o = L->tabS[s];
                w0 = L->d0[o];
                w1 = L->d1[o];
            }
            jj = w0.x + PR * (rank - s);
            lro = (w0.w >> 2) & 31u;
            if constexpr (SKIP) isp = jj == (w1.z & 0xFFFFFFu);
            if (jj < (uint32_t)NL) {  // (a probe task reads a slot no entry is in: only its end is used, set below)
                ent = L->e[WSLOT(lro, jj)][o];
            } else if constexpr (OPT & 2) {
                far = !isp;
            } else {
                const PIntv* obp = reinterpret_cast<const PIntv*>(P.scratch + (wown + o) * 2ull * cap);
                const uint32_t at = w0.z + jj;
                ent = *reinterpret_cast<const uint4*>(obp + (at < 2 * cap ? at : 0u));
            }
            if constexpr (PAIR) {
                has2 = jj + 1 < w1.z;
                if (has2) {
                    if (jj + 1 < (uint32_t)NL) {
                        ent2 = L->e[WSLOT(lro, jj + 1)][o];
                    } else if constexpr (OPT & 2) {
                        far2 = true;
                    } else {
                        const PIntv* obp = reinterpret_cast<const PIntv*>(P.scratch + (wown + o) * 2ull * cap);
                        const uint32_t at = w0.z + jj + 1;
                        ent2 = *reinterpret_cast<const uint4*>(obp + (at < 2 * cap ? at : 0u));
                    }
                }
            }
        }
        if constexpr (SKIP) {  // the probed string ends at i + dp
            if (isp) ent.w = ((w0.w >> 10) + (w1.z >> 24)) << 6;
        }
        const bool ld_q = qwant != qb && qwant != ~0u;
        if constexpr (!(OPT & 4)) WP_ISSUE();
        // entries beyond the LDS list: the owner's arena (the bound only guards a broken list), in a
        // wave-uniform branch that waits for them itself -- a wait at the join would run every
        // iteration, and one vmcnt counts the owners' result stores too (their acks, every iteration)
        if (OPT & 2 && __builtin_expect(__any(far || far2), 0)) {
            const PIntv* obp = reinterpret_cast<const PIntv*>(P.scratch + (wown + o) * 2ull * cap);
            if (far) {
                const uint32_t at = w0.z + jj;
                ent = *reinterpret_cast<const uint4*>(obp + (at < 2 * cap ? at : 0u));
            }
            if (PAIR && far2) {
                const uint32_t at = w0.z + jj + 1;
                ent2 = *reinterpret_cast<const uint4*>(obp + (at < 2 * cap ? at : 0u));
            }
            __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
        }
        // the extend: forward owners their own ik (a = x[1]), workers an entry backward (a = x[0])
        const bool task = worker || fwdreq;
        const uint64_t ra = fwdreq ? ik1 : p_x0(ent), rb = fwdreq ? ik0 : p_x1(ent), rs = fwdreq ? ik2 : p_x2(ent);
        const int rc = fwdreq ? cur_c : (int)(w0.w & 3u);
        const uint64_t k = ra - 1, l = k + rs;
        uint64_t kk = k - (k >= P.primary), ll = l - (l >= P.primary);
        // rows past the BWT only come from a broken entry: keep the loads inside the index
        // (the results then differ from the oracle instead of faulting the device)
        if (kk >= P.L2[4]) kk = 0;
        if (ll >= P.L2[4]) ll = 0;
        const uint32_t bk = (uint32_t)(kk >> 6), bl = (uint32_t)(ll >> 6);
        if constexpr (OPT & 4) {
            // the bucket indices exist here (the entry has landed) before anything below is issued
            asm volatile("" ::"v"(bk), "v"(bl) : "memory");
            WP_ISSUE();
        }
        uint4 k0 = WP_IDLE128(), k1 = WP_IDLE128(), l0 = WP_IDLE128(), l1 = WP_IDLE128();
        // KT: a result of at most K bases from the table (forward: q[x, i]; backward: q[i, end))
        bool ktp = false;
        if constexpr (SKIP) {  // the only probes: an owner's own (start / end of a call; the owner's block left
            // the slot in na), a step's last task (the dp bases from position i, of the descriptor's K)
            ktp = lane_flag(ownp || isp);
            if (ktp) k0 = P.kt[ownp ? (uint32_t)na : kt_slot(w1.w, (int)(w1.z >> 24), K, true)];
        } else if constexpr (KT) {
            if (task && K > 0) {
                const int lq = fwdreq ? i + 1 - x : (int)p_end(ent) - (int)(w0.w >> 10);
                if (lq <= K) {
                    const uint32_t code = fwdreq ? kc << 2 | (uint32_t)(3 - cur_c) : w1.w >> (2 * (K - lq));
                    const uint64_t base = ((1ull << (2 * lq)) - 4) / 3;
                    k0 = P.kt[base + code];
                    ktp = true;
                }
            }
        }
        if (task && !ktp) {
            const uint32_t *a0, *a1;
            block_chunks<false>(P.occ64, bk, a0, a1);
            k0 = *reinterpret_cast<const uint4*>(a0);
            k1 = *reinterpret_cast<const uint4*>(a1);
            if (bl != bk) {
                block_chunks<false>(P.occ64, bl, a0, a1);
                l0 = *reinterpret_cast<const uint4*>(a0);
                l1 = *reinterpret_cast<const uint4*>(a1);
            }
        }
        // PAIR: the lane's second entry (same base), its buckets in flight beside the first's
        uint64_t ra2 = 0, rb2 = 0, rs2 = 0, kk2 = 0, ll2 = 0;
        uint32_t bk2 = 0, bl2 = 0;
        uint4 m0 = {0, 0, 0, 0}, m1 = {0, 0, 0, 0}, n0 = {0, 0, 0, 0}, n1 = {0, 0, 0, 0};
        if constexpr (PAIR) {
            if (has2) {
                ra2 = p_x0(ent2), rb2 = p_x1(ent2), rs2 = p_x2(ent2);
                const uint64_t k2 = ra2 - 1, l2 = k2 + rs2;
                kk2 = k2 - (k2 >= P.primary), ll2 = l2 - (l2 >= P.primary);
                if (kk2 >= P.L2[4]) kk2 = 0;
                if (ll2 >= P.L2[4]) ll2 = 0;
                bk2 = (uint32_t)(kk2 >> 6), bl2 = (uint32_t)(ll2 >> 6);
                const uint32_t *a0, *a1;
                block_chunks<false>(P.occ64, bk2, a0, a1);
                m0 = *reinterpret_cast<const uint4*>(a0);
                m1 = *reinterpret_cast<const uint4*>(a1);
                if (bl2 != bk2) {
                    block_chunks<false>(P.occ64, bl2, a0, a1);
                    n0 = *reinterpret_cast<const uint4*>(a0);
                    n1 = *reinterpret_cast<const uint4*>(a1);
                }
            }
        }
        if constexpr (PRIO == 1) __builtin_amdgcn_s_setprio(0);
        // vmcnt(0) as the builtin, not inline asm: the compiler's wait insertion sees it and knows the
        // LDS-DMA above has landed (after an opaque asm wait it re-waited vmcnt(0) before the next
        // iteration's LDS reads, i.e. for the acks of the result stores)
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) expcnt(7) lgkmcnt(15)
        if (ld_q) {
            qv = L->q[me];
            qb = qwant;
        }
        if constexpr (SKIP) {  // one region: the few probe lanes take the table's entry by selects
            if (task) {
                const Bucket32 wk{k0, k1};
                const Bucket32 wl = bl != bk ? Bucket32{l0, l1} : wk;
                if constexpr (WIDE) extend_counts64<(DIET & 64) != 0>(P.primary, P.L2, ra, rb, rs, rc, kk, ll, wk, wl, na, nb, ns);
                else extend_counts32(P.primary, P.L2, ra, rb, rs, rc, kk, ll, wk, wl, na, nb, ns);
                // (the probe's sides as values of their own: with the unpacking left inside the selects' arms
                // they became a branch tree over ktp and fwdreq once the extend was the 32-bit one)
                const uint64_t t0 = p_x0(k0), t1 = p_x1(k0), t2 = p_x2(k0);
                const uint64_t ta = fwdreq ? t1 : t0, tb = fwdreq ? t0 : t1;
                na = ktp ? ta : na;
                nb = ktp ? tb : nb;
                ns = ktp ? t2 : ns;
            }
        } else if (ktp) {  // forward: na is the x[1] side, backward: the x[0] side
            na = fwdreq ? p_x1(k0) : p_x0(k0);
            nb = fwdreq ? p_x0(k0) : p_x1(k0);
            ns = p_x2(k0);
        } else if (task) {
            const Bucket32 wk{k0, k1};
            const Bucket32 wl = bl != bk ? Bucket32{l0, l1} : wk;
            extend_counts64<(DIET & 64) != 0>(P.primary, P.L2, ra, rb, rs, rc, kk, ll, wk, wl, na, nb, ns);
        }
        uint64_t na2 = 0, nb2 = 0, ns2 = 0;
        if constexpr (PAIR) {
            if (has2) {
                const Bucket32 wk{m0, m1};
                const Bucket32 wl = bl2 != bk2 ? Bucket32{n0, n1} : wk;
                extend_counts64<false>(P.primary, P.L2, ra2, rb2, rs2, rc, kk2, ll2, wk, wl, na2, nb2, ns2);
            }
        }
        // ---- the backward results: survive, dedup, rank, write into curr ----
        // entries of a segment in order: lane by lane, (PAIR) first then second entry
        const bool surv = worker && ns >= (uint64_t)w1.x;
        const bool surv2 = PAIR && has2 && ns2 >= (uint64_t)w1.x;
        const uint64_t smask = __ballot(surv);
        const uint64_t smask2 = PAIR ? (uint64_t)__ballot(surv2) : 0ull;
        RES[me] = PAIR && has2 ? ns2 : ns;  // the lane's last entry
        if constexpr (PAIR) L->res1[me] = ns;
        wave_lds_fence();
        bool keep = false;
        if (surv) {
            if (rank == s) {  // first entry of this chunk: against the last entry kept before it
                const uint64_t lx = (uint64_t)((w0.w >> 8) & 3u) << 32 | w1.y;
                keep = w0.y == 0 || ns != lx;
            } else {          // against the previous entry: the previous free lane's last one
                const int pp = hibit64(fmask & ((1ull << me) - 1ull));
                keep = !(((PAIR ? smask2 : smask) >> pp) & 1) || ns != RES[pp];
            }
        }
        const bool keep2 = surv2 && (!surv || ns2 != ns);
        const uint64_t kmask = __ballot(keep);
        const uint64_t kmask2 = PAIR ? (uint64_t)__ballot(keep2) : 0ull;
        if (keep || keep2) {
            const uint32_t pf = L->tabP[s];
            const uint64_t before = (1ull << me) - 1ull & ~((1ull << pf) - 1ull);
            const uint32_t kr = (uint32_t)(__popcll(kmask & before) + __popcll(kmask2 & before));
            PIntv* obp = reinterpret_cast<PIntv*>(P.scratch + (wown + o) * 2ull * cap);
            if (keep) {
                const uint32_t idx = w0.y + kr;
                const uint4 e = pack_p(na, nb, ns, p_end(ent));
                if (idx < (uint32_t)NL) L->e[WSLOT(lro, idx)][o] = e;
                else if (idx < cap) *reinterpret_cast<uint4*>(obp + cap + idx) = e;
            }
            if (PAIR && keep2) {
                const uint32_t idx = w0.y + kr + (keep ? 1u : 0u);
                const uint4 e = pack_p(na2, nb2, ns2, p_end(ent2));
                if (idx < (uint32_t)NL) L->e[WSLOT(lro, idx)][o] = e;
                else if (idx < cap) *reinterpret_cast<uint4*>(obp + cap + idx) = e;
            }
        }
        // ---- owners whose entries ran: the chunk's outcome ----
        if (take) {
            const uint32_t pf = L->tabP[excl], pl = L->tabP[excl + take - 1];
            const uint64_t seg = ((2ull << pl) - 1ull) & ~((1ull << pf) - 1ull);
            const uint64_t km = kmask & seg, km2 = kmask2 & seg;
            if (j == 0) fail0 = (SKIP ? fail0 & 2u : 0u) | !((smask >> pf) & 1);
            if (km | km2) {  // the last entry kept: the highest lane's second entry if it kept one
                const int hb = hibit64(km | km2);
                last_x2 = ((km2 >> hb) & 1) ? RES[hb] : (PAIR ? L->res1[hb] : RES[hb]);
            }
            curr_n += (uint32_t)(__popcll(km) + __popcll(km2));
            j += min(rem, PR * take);
            if (j == prev_n + (SKIP ? fail0 >> 1 : 0u)) phase = P_BWD_DONE;
        }
        wave_lds_fence();  // this iteration's LDS reads before the next one's writes
    }
#undef WP_EMIT
#undef WP_PUSH
#undef WP_VP
#undef WP_DP
#undef WP_OUT
#undef WP_IDLE32
#undef WP_IDLE128
#undef WSLOT
#undef QBLK
    if (P.tspan && me == 0) atomicMax(reinterpret_cast<unsigned long long*>(P.tspan) + 1, (unsigned long long)rtstamp());
}

template <int OWN, int NL, int PRIO, int WPE = 3, bool PAIR = false, bool KT = false, bool DPOS = false, int OPT = 15>
__global__ __launch_bounds__(256, WPE) void seed_wp_kernel(SeedParams P) {
    seed_wp_body<OWN, NL, PRIO, WPE, PAIR, KT, DPOS, OPT, false>(P);
}

// the same with the short entries virtual (SKIP; reads the k-mer table, every OPT bit)
template <int OWN, int NL, int PRIO, int WPE, bool WIDE = true>
__global__ __launch_bounds__(256, WPE) void seed_wp_kernel_skip(SeedParams P) {
    seed_wp_body<OWN, NL, PRIO, WPE, false, true, false, 15, true, WIDE>(P);
}

// Raw logs -> the lists smem_next2 returns: reverse each bwt_smem1 output
// (software/bwt.c:830) and merge matches with sub-matches keyed by
// (start, len - end) (software/bwamem.c:280-301).  The log holds only what
// the merge keeps (the seeding kernel applies :287-288's filter when it
// emits), so a read's records map one to one onto its output; a call's extent
// is the run of its ordinal, the match / sub-match split its tag bit
// (smem_kernels.h).
// Four threads per read, one per 8-B word of bwtintv_t: all four walk the
// same merge (on the info words) and each moves its own word, so a wave's
// loads and stores touch 16 intervals' lines instead of 64.  The per-read
// sizes come from the seeding kernel.
__global__ __launch_bounds__(256) void finalize_kernel(FinalizeParams F) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int r = (int)(t >> 2), w = (int)(t & 3);
    if (r >= F.n) return;
    const int s = F.ovf_slot ? F.ovf_slot[r] : -1;
    const Intv* raw = s >= 0 ? F.ovf_intv + (uint64_t)s * F.ovf_slot_intv : F.main_intv + (uint64_t)r * F.slot_intv;
    const uint32_t nraw = (uint32_t)F.sizes[2 * (uint64_t)r], nc = (uint32_t)F.sizes[2 * (uint64_t)r + 1];
    const uint32_t len = (uint32_t)(F.offs[r + 1] - F.offs[r]);
    const uint64_t* rw = reinterpret_cast<const uint64_t*>(raw);
    uint64_t* ow = reinterpret_cast<uint64_t*>(F.flat_intv + F.intv_off[r]);
    const uint64_t cout = F.call_off[r];
    const uint64_t wmask = w == 0 ? RAW_COORD_MASK : ~0ull;  // x0 sheds its tag
    uint32_t pos = 0;
    for (uint32_t c = 0; c < nc; ++c) {
        // the call's records: m_n matches, then s_n sub-matches (none at all: an empty list)
        uint32_t m_n = 0, s_n = 0;
        for (uint32_t k = pos; k < nraw; ++k) {
            const uint32_t tag = (uint32_t)(rw[(uint64_t)k * 4] >> RAW_ORD_SHIFT);
            if ((tag & RAW_ORD_MASK) != (c & RAW_ORD_MASK)) break;
            if (tag & RAW_SUB_BIT) ++s_n;
            else ++m_n;
        }
        // M[m_n-1-a] is the a-th match in final order; likewise S for sub-matches
        const uint64_t* M = rw + (uint64_t)pos * 4;
        const uint64_t* S = rw + (uint64_t)(pos + m_n) * 4;
        uint64_t* o = ow + (uint64_t)pos * 4 + w;
        uint32_t a = 0, b = 0;
        while (a < m_n || b < s_n) {
            bool take_m;
            if (b >= s_n) {
                take_m = true;
            } else if (a >= m_n) {
                take_m = false;
            } else {
                const uint64_t si = S[(uint64_t)(s_n - 1 - b) * 4 + 3];
                const uint64_t mi = M[(uint64_t)(m_n - 1 - a) * 4 + 3];
                const uint64_t xi = (mi >> 32 << 32) | (uint64_t)(uint32_t)(len - (uint32_t)mi);
                const uint64_t xj = (si >> 32 << 32) | (uint64_t)(uint32_t)(len - (uint32_t)si);
                take_m = (int64_t)xi < (int64_t)xj;
            }
            if (take_m) {
                *o = M[(uint64_t)(m_n - 1 - a) * 4 + w] & wmask;
                ++a;
            } else {
                *o = S[(uint64_t)(s_n - 1 - b) * 4 + w] & wmask;
                ++b;
            }
            o += 4;
        }
        if (w == 0) F.flat_calls[cout + c] = m_n + s_n;
        pos += m_n + s_n;
    }
}

__global__ void fill_i32_kernel(int32_t* p, int32_t v, int n) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) p[r] = v;
}

__global__ void ovf_slot_kernel(const int32_t* __restrict__ items, int n_ovf, int32_t* __restrict__ ovf_slot) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n_ovf) ovf_slot[items[s]] = s;
}

}  // namespace smem

// ------------------------------------------------------------ host launchers
// The product build instantiates the kernel a handle on its default runs (seed_wp_kernel
// variant 68: 49's shape with the short entries virtual; smem_gpu.cpp seed_run_variant),
// 49 itself (the plain kernel: a handle without a usable k-mer table, or 49 asked for by
// number), 49's k-mer table twin (54) and 68 with the extend's counts in 64 bits (71).  The
// other seed_wp_kernel shapes and OPT-bit twins (40-70 other than 49 / 54 / 68;
// DESIGN.md §5) are compiled only with SMEM_AB_VARIANTS (make AB=1): the
// library ships no kernel whose numbers are already recorded.  (Rounds 1-4's
// one-lane-per-read seed_kernel, variants 2-31, wrote the raw log format of
// its time and left with it; its numbers are in DESIGN.md §5.)
extern "C" int smem_seed_variant_built(int variant) {
#ifdef SMEM_AB_VARIANTS
    return variant == 0 || (variant >= 40 && variant <= 71);
#else
    return variant == 0 || variant == 49 || variant == 54 || variant == 68 || variant == 71;
#endif
}

extern "C" hipError_t smem_launch_seed(const smem::SeedParams* P, int grid, int block, int variant, hipStream_t st) {
    switch (variant) {
#ifdef SMEM_AB_VARIANTS
        // 40-43: the backward phase wave-parallel over list entries (seed_wp_kernel<owners per wave,
        // LDS list entries per owner, wave priority>)
        case 40: hipLaunchKernelGGL((smem::seed_wp_kernel<32, 20, 1>), dim3(grid), dim3(block), 0, st, *P); break;
        case 41: hipLaunchKernelGGL((smem::seed_wp_kernel<32, 16, 1>), dim3(grid), dim3(block), 0, st, *P); break;
        case 42: hipLaunchKernelGGL((smem::seed_wp_kernel<24, 24, 1>), dim3(grid), dim3(block), 0, st, *P); break;
        case 43: hipLaunchKernelGGL((smem::seed_wp_kernel<32, 20, 0>), dim3(grid), dim3(block), 0, st, *P); break;
        // 44-46: 4 blocks (16 waves) per CU with shorter lists: <24 owners, 16 entries>, <32, 12>, <28, 14>
        case 44: hipLaunchKernelGGL((smem::seed_wp_kernel<24, 16, 1, 4>), dim3(grid), dim3(block), 0, st, *P); break;
        case 45: hipLaunchKernelGGL((smem::seed_wp_kernel<32, 12, 1, 4>), dim3(grid), dim3(block), 0, st, *P); break;
        case 46: hipLaunchKernelGGL((smem::seed_wp_kernel<28, 14, 1, 4>), dim3(grid), dim3(block), 0, st, *P); break;
        // 47-48: two entries per worker lane (PAIR): <32, 20>, <24, 24> (3 blocks per CU)
        case 47: hipLaunchKernelGGL((smem::seed_wp_kernel<32, 20, 1, 3, true>), dim3(grid), dim3(block), 0, st, *P); break;
        case 48: hipLaunchKernelGGL((smem::seed_wp_kernel<24, 24, 1, 3, true>), dim3(grid), dim3(block), 0, st, *P); break;
        // 49-51: 4 blocks per CU: <24, 18>, <20, 22>, 44 without wave priority
        case 50: hipLaunchKernelGGL((smem::seed_wp_kernel<20, 22, 1, 4>), dim3(grid), dim3(block), 0, st, *P); break;
        case 51: hipLaunchKernelGGL((smem::seed_wp_kernel<24, 16, 0, 4>), dim3(grid), dim3(block), 0, st, *P); break;
        // 52-53: 4 blocks per CU: <24, 20>, <28, 16>
        case 52: hipLaunchKernelGGL((smem::seed_wp_kernel<24, 20, 1, 4>), dim3(grid), dim3(block), 0, st, *P); break;
        case 53: hipLaunchKernelGGL((smem::seed_wp_kernel<28, 16, 1, 4>), dim3(grid), dim3(block), 0, st, *P); break;
        // 55: with the k-mer table (KT; smem_gpu_set_kmer_table, no table: plain), 40's shape
        case 55: hipLaunchKernelGGL((smem::seed_wp_kernel<32, 20, 1, 3, false, true>), dim3(grid), dim3(block), 0, st, *P); break;
        // 56-57: descriptors by start position (DPOS): 49's shape, and with the k-mer table
        case 56: hipLaunchKernelGGL((smem::seed_wp_kernel<24, 18, 1, 4, false, false, true>), dim3(grid), dim3(block), 0, st, *P); break;
        case 57: hipLaunchKernelGGL((smem::seed_wp_kernel<24, 18, 1, 4, false, true, true>), dim3(grid), dim3(block), 0, st, *P); break;
        // 58-62: 49 with the memory-issue order taken apart (OPT bits, seed_wp_kernel): 58 none, 59 no
        // uniform arena branch, 60 the DMA / claim before the entry, 61 the claim when a read starts,
        // 62 the compiler's atomicAdd
        case 58: hipLaunchKernelGGL((smem::seed_wp_kernel<24, 18, 1, 4, false, false, false, 0>), dim3(grid), dim3(block), 0, st, *P); break;
        case 59: hipLaunchKernelGGL((smem::seed_wp_kernel<24, 18, 1, 4, false, false, false, 13>), dim3(grid), dim3(block), 0, st, *P); break;
        case 60: hipLaunchKernelGGL((smem::seed_wp_kernel<24, 18, 1, 4, false, false, false, 11>), dim3(grid), dim3(block), 0, st, *P); break;
        case 61: hipLaunchKernelGGL((smem::seed_wp_kernel<24, 18, 1, 4, false, false, false, 14>), dim3(grid), dim3(block), 0, st, *P); break;
        case 62: hipLaunchKernelGGL((smem::seed_wp_kernel<24, 18, 1, 4, false, false, false, 7>), dim3(grid), dim3(block), 0, st, *P); break;
        // 63-67: 49 with the instruction diet taken apart (OPT bits 16-128 take an arm out): 63 the idle
        // lanes' temporaries zeroed, 64 the `out` flag, 65 the selects by base as compare chains, 66 the
        // query byte by a compare chain, 67 none of the four (the kernel before the diet)
        case 63: hipLaunchKernelGGL((smem::seed_wp_kernel<24, 18, 1, 4, false, false, false, 31>), dim3(grid), dim3(block), 0, st, *P); break;
        case 64: hipLaunchKernelGGL((smem::seed_wp_kernel<24, 18, 1, 4, false, false, false, 47>), dim3(grid), dim3(block), 0, st, *P); break;
        case 65: hipLaunchKernelGGL((smem::seed_wp_kernel<24, 18, 1, 4, false, false, false, 79>), dim3(grid), dim3(block), 0, st, *P); break;
        case 66: hipLaunchKernelGGL((smem::seed_wp_kernel<24, 18, 1, 4, false, false, false, 143>), dim3(grid), dim3(block), 0, st, *P); break;
        case 67: hipLaunchKernelGGL((smem::seed_wp_kernel<24, 18, 1, 4, false, false, false, 255>), dim3(grid), dim3(block), 0, st, *P); break;
        // 69-70: 71 (virtual short entries, 64-bit counts) with more owners and shorter lists: <32, 12>, <28, 14>
        case 69: hipLaunchKernelGGL((smem::seed_wp_kernel_skip<32, 12, 1, 4>), dim3(grid), dim3(block), 0, st, *P); break;
        case 70: hipLaunchKernelGGL((smem::seed_wp_kernel_skip<28, 14, 1, 4>), dim3(grid), dim3(block), 0, st, *P); break;
#endif
        // 54: the default's shape with the k-mer table (KT; smem_gpu_set_kmer_table, no table: plain)
        case 54: hipLaunchKernelGGL((smem::seed_wp_kernel<24, 18, 1, 4, false, true>), dim3(grid), dim3(block), 0, st, *P); break;
        // 68: 49's shape with the short entries virtual (SKIP; no table: 49's path) and the extend's counts
        // in 32 bits; 71: the same with the counts in 64 bits (an index with 2^32 or more of one base, or
        // SMEM_GPU_OCC_WIDE=1; smem_gpu.cpp seed_run_variant)
        case 68: hipLaunchKernelGGL((smem::seed_wp_kernel_skip<24, 18, 1, 4, false>), dim3(grid), dim3(block), 0, st, *P); break;
        case 71: hipLaunchKernelGGL((smem::seed_wp_kernel_skip<24, 18, 1, 4, true>), dim3(grid), dim3(block), 0, st, *P); break;
        // 49 (and any number this build does not have): seed_wp_kernel<24 owners per wave, 18 LDS list
        // entries per owner, wave priority, 4 blocks per CU> with every OPT bit
        default: hipLaunchKernelGGL((smem::seed_wp_kernel<24, 18, 1, 4>), dim3(grid), dim3(block), 0, st, *P); break;
    }
    return hipGetLastError();
}

extern "C" hipError_t smem_launch_finalize(const smem::FinalizeParams* F, int write, hipStream_t st) {
    if (F->n <= 0 || !write) return hipSuccess;  // sizes come from the seeding kernel: no count pass
    const unsigned g = (unsigned)((4ull * F->n + 255) / 256);
    hipLaunchKernelGGL(smem::finalize_kernel, dim3(g), dim3(256), 0, st, *F);
    return hipGetLastError();
}

namespace smem {
// flat bwtintv_t (32 B) -> the 16-B wire entry smem_pintv_t (include/smem_gpu.h):
// x0, x1, x2 low words, then x0/x1/x2 bits 32-33 and the query begin / end
// (13 bits each: reads < 8192 bp, checked on the host)
__global__ __launch_bounds__(256) void pack_intv_kernel(const Intv* __restrict__ in, uint64_t n, uint4* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Intv v = in[i];
    const uint32_t beg = (uint32_t)(v.info >> 32), end = (uint32_t)v.info;
    out[i] = make_uint4((uint32_t)v.x0, (uint32_t)v.x1, (uint32_t)v.x2,
                        (uint32_t)(v.x0 >> 32) | (uint32_t)(v.x1 >> 32) << 2 | (uint32_t)(v.x2 >> 32) << 4 | beg << 6 |
                            end << 19);
}
}  // namespace smem

extern "C" hipError_t smem_launch_pack_intv(const smem::Intv* in, uint64_t n, uint4* out, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(smem::pack_intv_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, n, out);
    return hipGetLastError();
}

extern "C" hipError_t smem_launch_fill_i32(int32_t* p, int32_t v, int n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(smem::fill_i32_kernel, dim3((n + 255) / 256), dim3(256), 0, st, p, v, n);
    return hipGetLastError();
}

extern "C" hipError_t smem_launch_ovf_slot(const int32_t* items, int n_ovf, int32_t* ovf_slot, hipStream_t st) {
    if (n_ovf <= 0) return hipSuccess;
    hipLaunchKernelGGL(smem::ovf_slot_kernel, dim3((n_ovf + 255) / 256), dim3(256), 0, st, items, n_ovf, ovf_slot);
    return hipGetLastError();
}

// ---------------------------------------------------------------- scans
// Size -> offset scans with (almost) no LDS: three small launches (tile sums,
// one-block scan of the tile sums, tile rescans with carry-in), wave scans by
// shuffles and 32 B of LDS per block.  The persistent seeding kernel of
// another worker's chunk holds all but 4 KB of every CU's LDS; a library scan
// (16 KB+ of LDS per block) then waits for that whole kernel, and with it the
// chunk's copies and the next chunk (profiles/r02/stream/).
namespace smem {
constexpr int SCAN_T = 256, SCAN_I = 8, SCAN_TILE = SCAN_T * SCAN_I;

__device__ __forceinline__ uint64_t wave_incl_scan(uint64_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// exclusive prefix of this thread's SCAN_I elements within the block, and the block total
__device__ __forceinline__ uint64_t block_excl(uint64_t tsum, uint64_t& total) {
    __shared__ uint64_t ws[SCAN_T / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t inc = wave_incl_scan(tsum, lane);
    if (lane == 63) ws[w] = inc;
    __syncthreads();
    uint64_t before = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < SCAN_T / 64; ++k) {
        before += k < w ? ws[k] : 0;
        total += ws[k];
    }
    __syncthreads();  // ws is reused by the next call
    return before + inc - tsum;
}

__global__ __launch_bounds__(SCAN_T) void scan_tile_sums(const uint64_t* __restrict__ in, int stride, int n,
                                                         uint64_t* __restrict__ bsum) {
    const int64_t b0 = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_I;
    uint64_t t = 0;
#pragma unroll
    for (int k = 0; k < SCAN_I; ++k) t += b0 + k < n ? in[(b0 + k) * stride] : 0;
    uint64_t total;
    (void)block_excl(t, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one block: bsum[0..nb) -> exclusive offsets in place
__global__ __launch_bounds__(SCAN_T) void scan_tile_offsets(uint64_t* __restrict__ bsum, int nb) {
    uint64_t carry = 0;
    for (int base = 0; base < nb; base += SCAN_TILE) {
        const int b0 = base + (int)threadIdx.x * SCAN_I;
        uint64_t v[SCAN_I], t = 0;
#pragma unroll
        for (int k = 0; k < SCAN_I; ++k) {
            v[k] = b0 + k < nb ? bsum[b0 + k] : 0;
            t += v[k];
        }
        uint64_t total;
        uint64_t run = carry + block_excl(t, total);
#pragma unroll
        for (int k = 0; k < SCAN_I; ++k) {
            if (b0 + k < nb) bsum[b0 + k] = run;
            run += v[k];
        }
        carry += total;
    }
}

__global__ __launch_bounds__(SCAN_T) void scan_tiles(const uint64_t* __restrict__ in, int stride, int n,
                                                     const uint64_t* __restrict__ boff, uint64_t* __restrict__ out,
                                                     uint64_t* __restrict__ total_out) {
    const int64_t b0 = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_I;
    uint64_t v[SCAN_I], t = 0;
#pragma unroll
    for (int k = 0; k < SCAN_I; ++k) {
        v[k] = b0 + k < n ? in[(b0 + k) * stride] : 0;
        t += v[k];
    }
    uint64_t total;
    uint64_t run = boff[blockIdx.x] + block_excl(t, total);
    if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = 0;
#pragma unroll
    for (int k = 0; k < SCAN_I; ++k) {
        run += v[k];
        if (b0 + k < n) out[b0 + k + 1] = run;
        if (total_out && b0 + k == n - 1) *total_out = run;
    }
}
}  // namespace smem

// out[0] = 0, out[1..n] = inclusive sums of in[0], in[stride], .. in[(n-1) stride];
// temp == nullptr queries the temporary size into *temp_bytes; total != nullptr
// receives out[n] too (a word the caller copies back with its other scalars)
extern "C" hipError_t smem_launch_offsets_strided(const uint64_t* in, int stride, uint64_t* out, int n, void* temp,
                                                  size_t* temp_bytes, uint64_t* total, hipStream_t st) {
    const int nb = n > 0 ? (n + smem::SCAN_TILE - 1) / smem::SCAN_TILE : 1;
    if (temp == nullptr) {
        *temp_bytes = sizeof(uint64_t) * (size_t)(nb + 1);
        return hipSuccess;
    }
    if (*temp_bytes < sizeof(uint64_t) * (size_t)nb) return hipErrorInvalidValue;
    if (n <= 0) {
        hipError_t e = hipMemsetAsync(out, 0, sizeof(uint64_t), st);
        if (e == hipSuccess && total) e = hipMemsetAsync(total, 0, sizeof(uint64_t), st);
        return e;
    }
    uint64_t* bsum = static_cast<uint64_t*>(temp);
    hipLaunchKernelGGL(smem::scan_tile_sums, dim3(nb), dim3(smem::SCAN_T), 0, st, in, stride, n, bsum);
    hipLaunchKernelGGL(smem::scan_tile_offsets, dim3(1), dim3(smem::SCAN_T), 0, st, bsum, nb);
    hipLaunchKernelGGL(smem::scan_tiles, dim3(nb), dim3(smem::SCAN_T), 0, st, in, stride, n, bsum, out, total);
    return hipGetLastError();
}

extern "C" hipError_t smem_launch_offsets(const uint64_t* in, uint64_t* out, int n, void* temp, size_t* temp_bytes,
                                          hipStream_t st) {
    return smem_launch_offsets_strided(in, 1, out, n, temp, temp_bytes, nullptr, st);
}

namespace smem {
// reference interleaved buckets (software/bwtindex.c:128-150: 4 x u64 Occ +
// 8 x u32 symbols per 128) -> Occ64 (occ_rank.h: Bucket32, occ64_bucket); one thread per 64 symbols
__global__ __launch_bounds__(256) void occ64_kernel(const uint32_t* __restrict__ bwt, uint64_t n_ref,
                                                     uint32_t* __restrict__ out) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= 2 * n_ref) return;
    const Bucket32 v = occ64_bucket(bwt + (b >> 1) * 16, (uint32_t)(b & 1));
    uint4* o = reinterpret_cast<uint4*>(out + b * 8);
    o[0] = v.cnt;
    o[1] = v.sym;
}
}  // namespace smem

namespace smem {
// k-mer table level L from level L - 1: one thread per (L-1)-mer W extends
// its bi-interval backward by each base c (bwt_extend, software/bwt.c:416-429)
// and writes cW's entry at index c << 2(L-1) | code(W)
__global__ __launch_bounds__(256) void kmer_table_kernel(SeedParams P, uint4* __restrict__ kt, int L) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n_par = 1ull << (2 * (L - 1));
    if (w >= n_par) return;
    const uint4* par = kt + ((1ull << (2 * (L - 1))) - 4) / 3;
    uint4* lev = kt + ((1ull << (2 * L)) - 4) / 3;
    const uint4 e = par[w];
    const uint64_t a = p_x0(e), b = p_x1(e), s = p_x2(e);
    if (s == 0) {  // absent string: so are its extensions
        for (int c = 0; c < 4; ++c) lev[(uint64_t)c << (2 * (L - 1)) | w] = make_uint4(0, 0, 0, 0);
        return;
    }
    const uint64_t k = a - 1, l = k + s;
    const uint64_t kk = k - (k >= P.primary), ll = l - (l >= P.primary);
    const uint4* o = reinterpret_cast<const uint4*>(P.occ64);  // block b: o[2b] counts, o[2b + 1] symbols
    const Bucket32 vk{o[2 * (kk >> 6)], o[2 * (kk >> 6) + 1]}, vl{o[2 * (ll >> 6)], o[2 * (ll >> 6) + 1]};
    for (int c = 0; c < 4; ++c) {
        uint64_t na, nb, ns;
        extend_counts64<false>(P.primary, P.L2, a, b, s, c, kk, ll, vk, vl, na, nb, ns);
        lev[(uint64_t)c << (2 * (L - 1)) | w] = ns ? pack_p(na, nb, ns, 0) : make_uint4(0, 0, 0, 0);
    }
}

// the smallest interval size of table level L (0: a string of L bases is absent) into mn[L], which the
// host presets to ~0: each thread the minimum of a strided share, each wave one atomic
__global__ __launch_bounds__(256) void kmer_level_min_kernel(const uint4* __restrict__ kt, int L,
                                                             unsigned long long* __restrict__ mn) {
    const uint64_t n = 1ull << (2 * L);
    const uint4* lev = kt + (n - 4) / 3;
    unsigned long long m = ~0ull;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n; w += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long s = p_x2(lev[w]);
        m = s < m ? s : m;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long t = __shfl_xor(m, d, 64);
        m = t < m ? t : m;
    }
    if ((threadIdx.x & 63) == 0) atomicMin(mn + L, m);
}

// the same for level L + 1, which the table does not store: each thread extends the L-mers W of a strided
// share backward by each base (as kmer_table_kernel does for a stored level; an absent W contributes 0)
// and keeps the smallest size, nothing is written but the wave's one atomic into *mn_next (preset to ~0).
// The same four sizes tell whether level L is strict: a present W with an extension of its own size (the
// other three absent, W not at the text's start) sets *not_strict (preset to 0; null: not asked for).  The
// index holds both strands, so the backward extensions of every W are the forward ones of every rc(W)
__global__ __launch_bounds__(256) void kmer_next_level_min_kernel(SeedParams P, const uint4* __restrict__ kt, int L,
                                                                  unsigned long long* __restrict__ mn_next,
                                                                  unsigned long long* __restrict__ not_strict) {
    const uint64_t n = 1ull << (2 * L);
    const uint4* lev = kt + (n - 4) / 3;
    const uint4* o = reinterpret_cast<const uint4*>(P.occ64);  // block b: o[2b] counts, o[2b + 1] symbols
    unsigned long long m = ~0ull;
    bool eq = false;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n; w += (uint64_t)gridDim.x * blockDim.x) {
        const uint4 e = lev[w];
        const uint64_t a = p_x0(e), b = p_x1(e), s = p_x2(e);
        if (s == 0) {
            m = 0;
            continue;
        }
        const uint64_t k = a - 1, l = k + s;
        uint64_t kk = k - (k >= P.primary), ll = l - (l >= P.primary);
        if (kk >= P.L2[4]) kk = 0;  // (only a broken table: the loads stay inside the index)
        if (ll >= P.L2[4]) ll = 0;
        const Bucket32 vk{o[2 * (kk >> 6)], o[2 * (kk >> 6) + 1]}, vl{o[2 * (ll >> 6)], o[2 * (ll >> 6) + 1]};
        for (int c = 0; c < 4; ++c) {
            uint64_t na, nb, ns;
            extend_counts64<false>(P.primary, P.L2, a, b, s, c, kk, ll, vk, vl, na, nb, ns);
            m = ns < m ? ns : m;
            eq |= ns == s;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long t = __shfl_xor(m, d, 64);
        m = t < m ? t : m;
    }
    if ((threadIdx.x & 63) == 0) atomicMin(mn_next, m);
    if (not_strict && __any(eq) && (threadIdx.x & 63) == 0) atomicMax(not_strict, 1ull);
}

// Occ64 -> Occ192 (see rank192); one thread per 64-B line of 192 symbols
__global__ __launch_bounds__(256) void occ192_kernel(const uint32_t* __restrict__ occ64, uint64_t n_blocks,
                                                      uint64_t n_lines, uint32_t* __restrict__ out) {
    const uint64_t L = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (L >= n_lines) return;
    const uint4* o = reinterpret_cast<const uint4*>(occ64);  // block b: o[2b] counts, o[2b + 1] symbols
    const uint64_t b0 = 3 * L;
    uint4 sym[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) sym[i] = b0 + i < n_blocks ? o[2 * (b0 + i) + 1] : make_uint4(0, 0, 0, 0);
    uint64_t c, g, t;
    if (b0 + 1 < n_blocks) {
        const uint4 cnt = o[2 * (b0 + 1)];
        c = occ_cgt(cnt, 0), g = occ_cgt(cnt, 1), t = occ_cgt(cnt, 2);
    } else {  // the line's first block is the last one: counts through its end
        const uint4 cnt = o[2 * b0];
        uint32_t C, G, T;
        count_cgt4(sym[0], 63, C, G, T);
        c = occ_cgt(cnt, 0) + C, g = occ_cgt(cnt, 1) + G, t = occ_cgt(cnt, 2) + T;
    }
    uint32_t dC, dG, dT;
    count_cgt4(sym[1], 63, dC, dG, dT);
    uint4* w = reinterpret_cast<uint4*>(out) + 4 * L;
    w[0] = make_uint4((uint32_t)c, (uint32_t)g, (uint32_t)t,
                      (uint32_t)(c >> 32) | (uint32_t)(g >> 32) << 2 | (uint32_t)(t >> 32) << 4 | dC << 6 | dG << 13 |
                          dT << 20);
    w[1] = sym[0];
    w[2] = sym[1];
    w[3] = sym[2];
}
}  // namespace smem

extern "C" hipError_t smem_launch_kmer_table(const uint32_t* occ64, uint64_t primary, const uint64_t* L2, int k,
                                              uint4* kt, hipStream_t st) {
    if (k < 1 || k > 15) return hipErrorInvalidValue;
    smem::SeedParams P;
    memset(&P, 0, sizeof(P));
    P.occ64 = occ64;
    P.primary = primary;
    for (int c = 0; c < 5; ++c) P.L2[c] = L2[c];
    uint4 lev1[4];  // bwt_set_intv (software/bwt.h:80)
    for (int c = 0; c < 4; ++c)
        lev1[c] = smem::pack_p(L2[c] + 1, L2[3 - c] + 1, L2[c + 1] - L2[c], 0);
    hipError_t e = hipMemcpyAsync(kt, lev1, sizeof(lev1), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // lev1 is on this stack
    for (int L = 2; L <= k && e == hipSuccess; ++L) {
        const uint64_t n = 1ull << (2 * (L - 1));
        hipLaunchKernelGGL(smem::kmer_table_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, P, kt, L);
        e = hipGetLastError();
    }
    return e;
}

extern "C" hipError_t smem_launch_kmer_min(const uint4* kt, int k, unsigned long long* mn, hipStream_t st) {
    if (k < 1 || k > 15) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(mn, 0xFF, sizeof(unsigned long long) * (size_t)(k + 1), st);
    for (int L = 1; L <= k && e == hipSuccess; ++L) {
        const uint64_t n = 1ull << (2 * L);
        const unsigned grid = (unsigned)std::min<uint64_t>((n + 255) / 256, 4096);
        hipLaunchKernelGGL(smem::kmer_level_min_kernel, dim3(grid), dim3(256), 0, st, kt, L, mn);
        e = hipGetLastError();
    }
    return e;
}

extern "C" hipError_t smem_launch_kmer_min_next(const uint32_t* occ64, uint64_t primary, const uint64_t* L2, const uint4* kt,
                                                 int k, unsigned long long* mn_next, unsigned long long* not_strict,
                                                 hipStream_t st) {
    if (k < 1 || k > 14) return hipErrorInvalidValue;
    smem::SeedParams P;
    memset(&P, 0, sizeof(P));
    P.occ64 = occ64;
    P.primary = primary;
    for (int c = 0; c < 5; ++c) P.L2[c] = L2[c];
    hipError_t e = hipMemsetAsync(mn_next, 0xFF, sizeof(unsigned long long), st);
    if (e == hipSuccess && not_strict) e = hipMemsetAsync(not_strict, 0, sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    const uint64_t n = 1ull << (2 * k);
    const unsigned grid = (unsigned)std::min<uint64_t>((n + 255) / 256, 16384);
    hipLaunchKernelGGL(smem::kmer_next_level_min_kernel, dim3(grid), dim3(256), 0, st, P, kt, k, mn_next, not_strict);
    return hipGetLastError();
}

extern "C" hipError_t smem_launch_occ192(const uint32_t* occ64, uint64_t n_blocks, uint32_t* out, hipStream_t st) {
    const uint64_t n_lines = (n_blocks + 2) / 3;
    if (n_lines == 0) return hipSuccess;
    hipLaunchKernelGGL(smem::occ192_kernel, dim3((unsigned)((n_lines + 255) / 256)), dim3(256), 0, st, occ64, n_blocks,
                       n_lines, out);
    return hipGetLastError();
}

extern "C" hipError_t smem_launch_occ64(const uint32_t* bwt, uint64_t n_ref_buckets, uint32_t* out, hipStream_t st) {
    const uint64_t n = 2 * n_ref_buckets;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(smem::occ64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, bwt, n_ref_buckets, out);
    return hipGetLastError();
}

// ------------------------------------------------------------------ bwt_sa
// The SA lookup mem_insert_seed() does for every seed occurrence
// (software/bwamem.c:462-474): for each interval of the smem_next2 lists
// with seed length >= k and x2 <= max_occ, bwt_sa(bwt, x0 + j), j < x2
// (software/bwt.c:104-114): LF steps (bwt_invPsi, software/bwt.c:71-77)
// until the row is a multiple of sa_intv, then the sampled SA.  Each LF step
// is one rank in one Occ64 bucket: the symbol at the row and its count are in
// the same 32 B.
namespace smem {


// occurrences of each interval (software/bwamem.c:467)
__global__ __launch_bounds__(256) void sa_count_kernel(SaParams S) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= S.n_intv) return;
    const Intv v = S.intv[t];
    const int slen = (int)((uint32_t)v.info - (uint32_t)(v.info >> 32));
    S.n_occ_intv[t] = (slen < S.min_seed_len || v.x2 > S.max_occ) ? 0 : v.x2;
}

// rows x0 .. x0 + n - 1 of every interval at its occurrence offset
__global__ __launch_bounds__(256) void sa_fill_kernel(SaParams S) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= S.n_intv) return;
    const uint64_t o = S.occ_off[t], n = S.occ_off[t + 1] - o;
    const uint64_t x0 = S.intv[t].x0;
    for (uint64_t j = 0; j < n; ++j) S.kstart[o + j] = x0 + j;
}

// One lane per occurrence, occurrences dealt lane-strided.  Lanes of a wave
// walk different numbers of LF steps (0 .. sa_intv-1); a lane that finishes
// takes its next occurrence in the same loop.  Every iteration makes exactly
// two 16-B loads per lane from per-lane addresses — the Occ64 bucket (counts,
// symbols) for a lane that steps, or the 16 B around its SA sample and
// around its next occurrence's row for a lane that finishes — so the wave
// waits for one memory round trip per iteration whatever its lanes do.
__global__ __launch_bounds__(256) void sa_walk_kernel(SaParams S) {
    const uint64_t lanes = (uint64_t)gridDim.x * blockDim.x;
    uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t mask = (1ull << S.sa_shift) - 1;
    const uint4* occ = reinterpret_cast<const uint4*>(S.occ64);
    const uint4* sa16 = reinterpret_cast<const uint4*>(S.sa);
    const uint4* ks16 = reinterpret_cast<const uint4*>(S.kstart);
    bool live = o < S.n_occ;
    uint64_t k = live ? S.kstart[o] : 0, steps = 0;
    while (__any(live)) {
        const bool step = live && (k & mask) != 0;
        const uint64_t on = o + lanes;  // next occurrence of this lane
        const uint64_t kk = k - (k > S.primary);
        const uint4* pa = step ? occ + (kk >> 6) * 2 : sa16 + ((k >> S.sa_shift) >> 1);
        const uint4* pb = step ? pa + 1 : ks16 + ((on < S.n_occ ? on : 0) >> 1);
        uint4 va = {0, 0, 0, 0}, vb = {0, 0, 0, 0};
        if (live) {
            va = *pa;
            vb = *pb;
        }
        if (step) {  // bwt_invPsi (software/bwt.c:71-77) on the Occ64 bucket
            if (k == S.primary) {
                k = 0;
            } else {
                const uint32_t pos = (uint32_t)(kk & 63);
                const int c = sym_at(vb, pos);
                uint32_t C, G, T;
                count_cgt4(vb, pos, C, G, T);
                const uint64_t oc = occ_cgt(va, 0) + C, og = occ_cgt(va, 1) + G, ot = occ_cgt(va, 2) + T;
                const uint64_t n = c == 0 ? kk + 1 - oc - og - ot : (c == 1 ? oc : (c == 2 ? og : ot));
                k = sel4(c, S.L2[0], S.L2[1], S.L2[2], S.L2[3]) + n;
            }
            ++steps;
        } else if (live) {
            // sa[0] = -1: unsigned wrap as in software/bwt.c:110-113
            const uint64_t si = k >> S.sa_shift;
            S.pos[o] = steps + ((si & 1) ? ((uint64_t)va.w << 32 | va.z) : ((uint64_t)va.y << 32 | va.x));
            o = on;
            live = o < S.n_occ;
            k = (o & 1) ? ((uint64_t)vb.w << 32 | vb.z) : ((uint64_t)vb.y << 32 | vb.x);
            steps = 0;
        }
    }
}

// A denser device copy of the sampled SA: dense[i] = bwt_sa(i * D) for
// D = 2^dshift dividing sa_intv, each computed by the same LF walk to the
// next stored sample.  bwt_sa(k) walked to the first multiple of D and
// finished from dense[] equals the reference's walk to the first multiple of
// sa_intv (same steps, same unsigned arithmetic, sa[0] = -1 included), so
// lookups take (D-1)/2 steps on average instead of (sa_intv-1)/2.
__global__ __launch_bounds__(256) void sa_densify_kernel(SaParams S, uint32_t dshift, uint64_t n_dense,
                                                          uint64_t* __restrict__ dense) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_dense) return;
    const uint64_t mask = (1ull << S.sa_shift) - 1;
    const uint4* occ = reinterpret_cast<const uint4*>(S.occ64);
    uint64_t k = i << dshift, steps = 0;
    while (k & mask) {
        if (k == S.primary) {
            k = 0;
        } else {
            const uint64_t kk = k - (k > S.primary);
            const uint4 va = occ[(kk >> 6) * 2], vb = occ[(kk >> 6) * 2 + 1];
            const uint32_t pos = (uint32_t)(kk & 63);
            const int c = sym_at(vb, pos);
            uint32_t C, G, T;
            count_cgt4(vb, pos, C, G, T);
            const uint64_t oc = occ_cgt(va, 0) + C, og = occ_cgt(va, 1) + G, ot = occ_cgt(va, 2) + T;
            const uint64_t n = c == 0 ? kk + 1 - oc - og - ot : (c == 1 ? oc : (c == 2 ? og : ot));
            k = sel4(c, S.L2[0], S.L2[1], S.L2[2], S.L2[3]) + n;
        }
        ++steps;
    }
    dense[i] = steps + S.sa[k >> S.sa_shift];
}

// The same dense[] in two passes that share the walks.  The walk from row
// i * D passes through other multiples of D on its way to a stored sample,
// and every dense row's walk from there on is that row's own walk, so:
//   hop pass:   every dense row that is not a stored sample walks only to the
//               next multiple of D: link[i] = (that row / D) | steps << 32.
//               The walks end at the first dense row, so together they step
//               over each BWT row once: seq_len LF steps instead of
//               n_dense * (sa_intv / D) * ~(D - 1).
//   chase pass: dense[i] = the steps summed along the links up to a stored
//               sample + that sample (unsigned, sa[0] = -1 wrapping as in
//               software/bwt.c:110-113), one 8-B load per link; a finished
//               row's link is replaced by its total (path compression), so
//               chains that reach it later stop there.
// Walks and chains differ in length across the lanes of a wave, so both
// passes deal their rows lane-strided and a lane that finishes takes its
// next row in the same loop (the sa_walk_kernel scheme).  Link targets need
// 32 bits: the host uses these passes while n_dense < 2^32.
__global__ __launch_bounds__(256) void sa_densify_hop_kernel(SaParams S, uint32_t dshift, uint64_t n_dense,
                                                              uint64_t* __restrict__ link) {
    const uint64_t lanes = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t smask = (1ull << (S.sa_shift - dshift)) - 1;  // dense rows that are stored samples
    const uint64_t dmask = (1ull << dshift) - 1;
    const uint4* occ = reinterpret_cast<const uint4*>(S.occ64);
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool live = i < n_dense;
    uint64_t k = i << dshift, steps = 0;
    while (__any(live)) {
        if (live && ((i & smask) == 0 || (steps && (k & dmask) == 0))) {
            if (i & smask) link[i] = (k >> dshift) | steps << 32;
            i += lanes;
            live = i < n_dense;
            k = i << dshift;
            steps = 0;
        } else if (live) {  // bwt_invPsi (software/bwt.c:71-77) on the Occ64 bucket
            if (k == S.primary) {
                k = 0;
            } else {
                const uint64_t kk = k - (k > S.primary);
                const uint4 va = occ[(kk >> 6) * 2], vb = occ[(kk >> 6) * 2 + 1];
                const uint32_t pos = (uint32_t)(kk & 63);
                const int c = sym_at(vb, pos);
                uint32_t C, G, T;
                count_cgt4(vb, pos, C, G, T);
                const uint64_t oc = occ_cgt(va, 0) + C, og = occ_cgt(va, 1) + G, ot = occ_cgt(va, 2) + T;
                const uint64_t n = c == 0 ? kk + 1 - oc - og - ot : (c == 1 ? oc : (c == 2 ? og : ot));
                k = sel4(c, S.L2[0], S.L2[1], S.L2[2], S.L2[3]) + n;
            }
            ++steps;
        }
    }
}

__global__ __launch_bounds__(256) void sa_densify_chase_kernel(SaParams S, uint32_t dshift, uint64_t n_dense,
                                                                uint64_t* link, uint64_t* __restrict__ dense) {
    const uint64_t lanes = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t rshift = S.sa_shift - dshift;
    const uint64_t smask = (1ull << rshift) - 1;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool live = i < n_dense;
    uint64_t j = i, acc = 0;
    while (__any(live)) {
        if (live && (j & smask) == 0) {
            dense[i] = acc + S.sa[j >> rshift];
            // path compression: a later chain through row i jumps straight to
            // the sample (its link still says "acc steps to row j", the same
            // walk).  Other lanes may read link[i] before or after this store
            // (an aligned 8-B store, never torn), and either value is right.
            if (acc) link[i] = j | acc << 32;
            i += lanes;
            live = i < n_dense;
            j = i;
            acc = 0;
        } else if (live) {
            const uint64_t l = link[j];
            acc += l >> 32;
            j = (uint32_t)l;
        }
    }
}

}  // namespace smem

// lane-strided passes: enough waves to fill the chip several times over
static unsigned densify_grid(uint64_t n) {
    const uint64_t want = (n + 255) / 256;
    return (unsigned)(want < 256 * 64 ? (want ? want : 1) : 256 * 64);
}

extern "C" hipError_t smem_launch_sa_densify2(const smem::SaParams* S, uint32_t dshift, uint64_t n_dense,
                                              uint64_t* link, uint64_t* dense, unsigned max_blocks, hipStream_t st) {
    if (n_dense == 0) return hipSuccess;
    if (n_dense >= (1ull << 32) || dshift >= S->sa_shift) return hipErrorInvalidValue;
    unsigned grid = densify_grid(n_dense);
    if (max_blocks && grid > max_blocks) grid = max_blocks;
    hipLaunchKernelGGL(smem::sa_densify_hop_kernel, dim3(grid), dim3(256), 0, st, *S, dshift, n_dense, link);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(smem::sa_densify_chase_kernel, dim3(grid), dim3(256), 0, st, *S, dshift, n_dense, link,
                       dense);
    return hipGetLastError();
}

extern "C" hipError_t smem_launch_sa_densify(const smem::SaParams* S, uint32_t dshift, uint64_t n_dense,
                                             uint64_t* dense, hipStream_t st) {
    if (n_dense == 0) return hipSuccess;
    hipLaunchKernelGGL(smem::sa_densify_kernel, dim3((unsigned)((n_dense + 255) / 256)), dim3(256), 0, st, *S, dshift,
                       n_dense, dense);
    return hipGetLastError();
}

extern "C" hipError_t smem_launch_sa_count(const smem::SaParams* S, hipStream_t st) {
    if (S->n_intv == 0) return hipSuccess;
    hipLaunchKernelGGL(smem::sa_count_kernel, dim3((unsigned)((S->n_intv + 255) / 256)), dim3(256), 0, st, *S);
    return hipGetLastError();
}

extern "C" hipError_t smem_launch_sa_walk(const smem::SaParams* S, int grid, hipStream_t st) {
    if (S->n_occ == 0) return hipSuccess;
    hipLaunchKernelGGL(smem::sa_fill_kernel, dim3((unsigned)((S->n_intv + 255) / 256)), dim3(256), 0, st, *S);
    hipLaunchKernelGGL(smem::sa_walk_kernel, dim3(grid), dim3(256), 0, st, *S);
    return hipGetLastError();
}

// this file's code object loaded on the current device without running
// anything (smem_gpu_reserve_slots: the first batch does not pay the load)
extern "C" hipError_t smem_preload_seed(void) {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&smem::sa_count_kernel));
}
