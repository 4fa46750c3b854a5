// occ_rank.h — the Occ64 bucket and the rank arithmetic of one bwt_extend on it, as host + device
// inlines: the kernels of smem_kernels.hip and the host twins of smem_gpu.cpp (smem_occ64_host,
// smem_extend_host) run the same code, so the arithmetic is tested without a GPU on counts no small
// index reaches.  Not part of the public C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define OCC_HD __host__ __device__ __forceinline__

namespace smem {

// one of four by a compare chain (the SA walk and the table builders; in seed_wp_kernel only the A/B
// twin of sel4b below)
OCC_HD uint64_t sel4(int c, uint64_t a, uint64_t b, uint64_t d, uint64_t e) {
    return c == 0 ? a : (c == 1 ? b : (c == 2 ? d : e));
}

// sel4 as two bit tests of c (0..3): v_cndmask only, where the compare chain above becomes a branch tree
OCC_HD uint64_t sel4b(int c, uint64_t a, uint64_t b, uint64_t d, uint64_t e) {
    const bool b0 = c & 1, b1 = c & 2;
    const uint64_t lo = b0 ? b : a, hi = b0 ? e : d;
    return b1 ? hi : lo;
}
OCC_HD uint32_t sel4b32(int c, uint32_t a, uint32_t b, uint32_t d, uint32_t e) {
    const bool b0 = c & 1, b1 = c & 2;
    const uint32_t lo = b0 ? b : a, hi = b0 ? e : d;
    return b1 ? hi : lo;
}

// ---- Occ64: the index re-laid for the GPU as one 32-B bucket per 64 BWT
// symbols (same 0.5 B/symbol as the reference's 64 B per 128).  Words 0-2:
// Occ(C), Occ(G), Occ(T) before the bucket, low 32 bits; word 3: their bits
// 32-33 (C | G << 2 | T << 4); words 4-7: the 64 symbols as two bit planes,
// plane L in words 4-5 (bit i of the 64-bit word = bit 0 of symbol i's 2-bit
// code, symbol 0 at bit 0 of word 4) and plane H in words 6-7 (bit 1 of the
// code), so C = L & ~H, G = ~L & H, T = L & H.  Occ(A) is implied: the $ row
// is not in the BWT, so A + C + G + T = position.  A rank then reads one 32-B
// bucket, masks both planes by one shift and popcounts three 64-bit words.
// The layout is the device's own: made at load (occ64_kernel), read by nothing
// outside csrc/.
struct Bucket32 {
    uint4 cnt, sym;
};

OCC_HD uint64_t occ_cgt(const uint4& c, int i) {
    const uint32_t lo = i == 0 ? c.x : (i == 1 ? c.y : c.z);
    return (uint64_t)((c.w >> (2 * i)) & 3) << 32 | lo;
}

OCC_HD uint64_t plane_l(const uint4& v) { return (uint64_t)v.y << 32 | v.x; }
OCC_HD uint64_t plane_h(const uint4& v) { return (uint64_t)v.w << 32 | v.z; }

// C, G, T among the first pos+1 (pos < 64) symbols of the bucket
OCC_HD void count_cgt4(const uint4& v, uint32_t pos, uint32_t& C, uint32_t& G, uint32_t& T) {
    const uint64_t m = ~0ull >> (63u - pos);
    const uint64_t l = plane_l(v) & m, h = plane_h(v) & m;
    T = (uint32_t)__builtin_popcountll(l & h);
    C = (uint32_t)__builtin_popcountll(l) - T;
    G = (uint32_t)__builtin_popcountll(h) - T;
}

// the symbol at pos (pos < 64)
OCC_HD int sym_at(const uint4& v, uint32_t pos) {
    return (int)((plane_l(v) >> pos) & 1u) | (int)((plane_h(v) >> pos) & 1u) << 1;
}

// 16 MSB-first 2-bit symbols of a reference word (software/bwt.h:71-78) -> their low and high bits,
// the word's first symbol at bit 0 (runs once per index, at load)
OCC_HD void planes16(uint32_t w, uint32_t& l, uint32_t& h) {
    l = 0, h = 0;
    for (int j = 0; j < 16; ++j) {
        const uint32_t s = (w >> ((15 - j) << 1)) & 3u;
        l |= (s & 1u) << j;
        h |= (s >> 1) << j;
    }
}

// Occ64 bucket `half` (0 / 1) of one reference bucket r (software/bwtindex.c:128-150: 4 x u64 Occ +
// 8 x u32 symbols per 128 symbols)
OCC_HD Bucket32 occ64_bucket(const uint32_t* r, uint32_t half) {
    uint64_t c1 = (uint64_t)r[3] << 32 | r[2], c2 = (uint64_t)r[5] << 32 | r[4], c3 = (uint64_t)r[7] << 32 | r[6];
    uint32_t l[8], h[8];
    for (int i = 0; i < 8; ++i) planes16(r[8 + i], l[i], h[i]);
    if (half) {  // add the first 64 symbols of the 128-block
        for (int i = 0; i < 4; ++i) {
            const uint32_t t = (uint32_t)__builtin_popcount(l[i] & h[i]);
            c1 += (uint32_t)__builtin_popcount(l[i]) - t;
            c2 += (uint32_t)__builtin_popcount(h[i]) - t;
            c3 += t;
        }
    }
    const uint32_t* pl = l + 4 * half;
    const uint32_t* ph = h + 4 * half;
    Bucket32 o;
    o.cnt = make_uint4((uint32_t)c1, (uint32_t)c2, (uint32_t)c3,
                       (uint32_t)(c1 >> 32) | (uint32_t)(c2 >> 32) << 2 | (uint32_t)(c3 >> 32) << 4);
    o.sym = make_uint4(pl[0] | pl[1] << 16, pl[2] | pl[3] << 16, ph[0] | ph[1] << 16, ph[2] | ph[3] << 16);
    return o;
}

// every base occurs fewer than 2^32 times in the BWT: extend_counts32 is exact (see there)
OCC_HD bool occ_narrow_ok(const uint64_t L2[5]) {
    bool ok = true;
    for (int c = 0; c < 4; ++c) ok = ok && L2[c + 1] - L2[c] < (1ull << 32);
    return ok;
}

// One bwt_extend in one direction on Occ64 buckets, returning only the child for
// base c, from the buckets of k = a-1 and l = k+s (kk, ll: the same rows without the $ row):
//   a: coordinate searched through the BWT (x[1] forward, x[0] backward), b: the other, s: the size
//   -> na = L2[c] + 1 + Occ(c, k), ns = Occ(c, l) - Occ(c, k),
//      nb = b + [$ in interval] + sum_{c' > c} (Occ(c', l) - Occ(c', k))
// (software/bwt.c:416-429; the four-way cumulative in :425-428 restricted to the child taken).
// tk1..3 / tl1..3: Occ(C / G / T) at k and at l.
// BSEL: the selects by c as bit tests (sel4b) and the sum over c' > c as suffix sums
template <bool BSEL>
OCC_HD void extend_from_occ(uint64_t primary, const uint64_t* L2, uint64_t a, uint64_t b, uint64_t s, int c, uint64_t kk,
                            uint64_t ll, uint64_t tk1, uint64_t tk2, uint64_t tk3, uint64_t tl1, uint64_t tl2,
                            uint64_t tl3, uint64_t& na, uint64_t& nb, uint64_t& ns) {
    const uint64_t tk0 = kk + 1 - tk1 - tk2 - tk3, tl0 = ll + 1 - tl1 - tl2 - tl3;
    const uint64_t d0 = tl0 - tk0, d1 = tl1 - tk1, d2 = tl2 - tk2, d3 = tl3 - tk3;
    if constexpr (BSEL) {  // the selects by c's two bits; the suffix sums once, then one select
        const uint64_t L2c = sel4b(c, L2[0], L2[1], L2[2], L2[3]);
        na = L2c + 1 + sel4b(c, tk0, tk1, tk2, tk3);
        ns = sel4b(c, d0, d1, d2, d3);
        const uint64_t g2 = d2 + d3, g1 = d1 + g2;
        nb = b + (uint64_t)(a <= primary && a + s - 1 >= primary) + sel4b(c, g1, g2, d3, 0);
        return;
    }
    const uint64_t L2c = sel4(c, L2[0], L2[1], L2[2], L2[3]);
    na = L2c + 1 + sel4(c, tk0, tk1, tk2, tk3);
    ns = sel4(c, d0, d1, d2, d3);
    const uint64_t gt = (c < 1 ? d1 : 0) + (c < 2 ? d2 : 0) + (c < 3 ? d3 : 0);
    nb = b + (uint64_t)(a <= primary && a + s - 1 >= primary) + gt;
}

template <bool BSEL = false>
OCC_HD void extend_counts64(uint64_t primary, const uint64_t* L2, uint64_t a, uint64_t b, uint64_t s, int c, uint64_t kk,
                            uint64_t ll, const Bucket32& vk, const Bucket32& vl, uint64_t& na, uint64_t& nb,
                            uint64_t& ns) {
    uint32_t Ck, Gk, Tk, Cl, Gl, Tl;
    count_cgt4(vk.sym, (uint32_t)(kk & 63), Ck, Gk, Tk);
    count_cgt4(vl.sym, (uint32_t)(ll & 63), Cl, Gl, Tl);
    extend_from_occ<BSEL>(primary, L2, a, b, s, c, kk, ll, occ_cgt(vk.cnt, 0) + Ck, occ_cgt(vk.cnt, 1) + Gk,
                          occ_cgt(vk.cnt, 2) + Tk, occ_cgt(vl.cnt, 0) + Cl, occ_cgt(vl.cnt, 1) + Gl,
                          occ_cgt(vl.cnt, 2) + Tl, na, nb, ns);
}

// The same with the counts in 32 bits, valid when every base occurs fewer than 2^32 times in the BWT
// (occ_narrow_ok).  Then every Occ(c, .) is below 2^32 (the headers' bits 32-33 are zero and the low
// words plus the popcounts do not wrap), and an interval of a non-empty string is within one base's rows,
// so its size and every partial sum of the four child sizes are below 2^32 too.  The child sizes are
// differences of the low words; Occ(A, .) is taken mod 2^32 from the low word of the row (exact: it is
// below 2^32); the child's start is the only 34-bit result, L2[c] + 1 plus a 32-bit addend.  Selects by
// c's two bits only (sel4b32).  Not for the empty string's interval (the k-mer table's first level).
OCC_HD void extend_counts32(uint64_t primary, const uint64_t* L2, uint64_t a, uint64_t b, uint64_t s, int c, uint64_t kk,
                            uint64_t ll, const Bucket32& vk, const Bucket32& vl, uint64_t& na, uint64_t& nb,
                            uint64_t& ns) {
    uint32_t Ck, Gk, Tk, Cl, Gl, Tl;
    count_cgt4(vk.sym, (uint32_t)(kk & 63), Ck, Gk, Tk);
    count_cgt4(vl.sym, (uint32_t)(ll & 63), Cl, Gl, Tl);
    const uint32_t k1 = vk.cnt.x + Ck, k2 = vk.cnt.y + Gk, k3 = vk.cnt.z + Tk;
    const uint32_t l1 = vl.cnt.x + Cl, l2 = vl.cnt.y + Gl, l3 = vl.cnt.z + Tl;
    const uint32_t k0 = (uint32_t)kk + 1u - k1 - k2 - k3;
    const uint32_t d1 = l1 - k1, d2 = l2 - k2, d3 = l3 - k3;
    const uint32_t d0 = (uint32_t)ll - (uint32_t)kk - d1 - d2 - d3;
    const uint32_t g2 = d2 + d3, g1 = d1 + g2;
    na = sel4b(c, L2[0], L2[1], L2[2], L2[3]) + 1 + (uint64_t)sel4b32(c, k0, k1, k2, k3);
    ns = sel4b32(c, d0, d1, d2, d3);
    nb = b + (uint64_t)(a <= primary && a + s - 1 >= primary) + (uint64_t)sel4b32(c, g1, g2, d3, 0u);
}

}  // namespace smem
