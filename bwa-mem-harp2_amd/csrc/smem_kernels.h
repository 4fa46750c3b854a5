// smem_kernels.h — device-side parameter blocks shared by smem_kernels.hip
// (kernels) and smem_gpu.cpp (runtime).  Not part of the public C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace smem {

// bwtintv_t (software/bwt.h:60-62)
struct Intv {
    uint64_t x0, x1, x2, info;
};

// A raw log record is a bwtintv_t whose x0 word also carries, above the 34-bit
// coordinate, where the record belongs in the read's output: bits 34-62 the
// ordinal of its smem_next2 call within the read (one call per base at most,
// reads <= 2^24 bases), bit 63 set for a sub-match of the call's re-seeding
// pass.  A call's records are contiguous: its matches, then the sub-matches
// the merge keeps, each run in the order bwt_smem1 pushed it (the reverse of
// its final order).  x1, x2 and info are bwtintv_t's.
constexpr int RAW_ORD_SHIFT = 34;
constexpr uint64_t RAW_COORD_MASK = (1ull << RAW_ORD_SHIFT) - 1;
constexpr uint32_t RAW_ORD_MASK = (1u << 29) - 1;   // of x0 >> RAW_ORD_SHIFT
constexpr uint32_t RAW_SUB_BIT = 1u << 29;          // of x0 >> RAW_ORD_SHIFT

struct SeedParams {
    const uint32_t* bwt;       // interleaved BWT + Occ, resident in HBM (reference layout)
    const uint32_t* occ64;     // the same index as 32-B buckets per 64 symbols (smem_launch_occ64)
    const uint32_t* occ192;    // the same index as 64-B lines of 192 symbols (smem_launch_occ192; variant 10)
    uint64_t primary;
    uint64_t L2[5];
    const uint8_t* codes;      // reads, concatenated nt4 codes (+32 B pad)
    const uint64_t* offs;      // n_reads + 1
    const int32_t* read_ids;   // work item -> read (nullptr: identity)
    int n_items;
    int min_seed_len, split_len_init, split_width, start_width;
    Intv* out_intv;            // raw logs [item][slot_intv], 64-B aligned
    uint32_t cap_intv;         // records a read may log; one more sends it to the overflow pass
    uint32_t slot_intv;        // cap_intv rounded up to even: record pairs are whole 64-B lines
    uint64_t* sizes;           // [read][2] intervals, smem_next2 lists of the read (one 16-B store;
                               // the compaction scans read it with stride 2); not written for a
                               // read that overflowed
    int32_t* ovf_count;
    int32_t* ovf_items;
    int32_t* head;             // work counter, zeroed before each launch
    uint4* scratch;            // per lane: 2 * cap_list packed 16-B list entries
    uint32_t cap_list;
    int dbg;                   // debug switches (0 in production)
    uint64_t* dbg_buf;         // stamped diagnostic variant: 8 x u64 per wave
    uint64_t* tspan;           // [0] max of ~(wave start), [1] max of wave end (s_memrealtime), nullptr: none
    const uint4* kt;           // k-mer bi-interval table (smem_launch_kmer_table; variant 23), nullptr: none
    int kt_k;                  // its longest k-mer: every level the table stores, a leaf level included
    int kt_dp0, kt_dp1;        // seed_wp_kernel SKIP: the probe depth of calls with min_intv = start_width and of
                               // re-seeding calls (min_intv <= split_width + 1): smem_kmer_probe_depth, <= kt_k; 0: none
};

// bwt_sa over the seeding output (software/bwamem.c:462-474, software/bwt.c:104-114)
struct SaParams {
    const uint32_t* occ64;
    uint64_t primary;
    uint64_t L2[5];
    const uint64_t* sa;        // sampled SA, sa[0] = -1
    uint32_t sa_shift;         // log2(sa_intv)
    const Intv* intv;          // flat smem_next2 intervals
    uint64_t n_intv;
    const uint64_t* occ_off;   // [n_intv + 1] exclusive prefix of occurrences per interval
    uint64_t n_occ;
    int min_seed_len;
    uint64_t max_occ;
    uint64_t* n_occ_intv;      // [n_intv] occurrences per interval (count kernel output)
    uint64_t* kstart;          // [n_occ + 2] the row of each occurrence (fill kernel)
    uint64_t* pos;             // [n_occ] bwt_sa results
};

// raw logs -> final smem_next2 lists (reverse + ordered merge, software/bwamem.c:280-301)
struct FinalizeParams {
    int n;
    const uint64_t* offs;          // read lengths for the merge key
    const uint64_t* sizes;         // [read][2] intervals (= raw records), lists
    const Intv* main_intv;
    uint32_t slot_intv;            // records per read slot
    const int32_t* ovf_slot;       // [read] slot in ovf_intv, -1: main; nullptr: no read overflowed
    const Intv* ovf_intv;
    uint32_t ovf_slot_intv;
    const uint64_t* intv_off;
    const uint64_t* call_off;
    Intv* flat_intv;
    uint32_t* flat_calls;
};

}  // namespace smem

extern "C" {
hipError_t smem_launch_seed(const smem::SeedParams* P, int grid, int block, int variant, hipStream_t st);
// 1 when this build instantiates seeding-kernel variant `variant` (A/B variants need SMEM_AB_VARIANTS)
int smem_seed_variant_built(int variant);
// reference interleaved words (n_ref_buckets x 64 B) -> 2 * n_ref_buckets 32-B buckets
hipError_t smem_launch_occ64(const uint32_t* bwt, uint64_t n_ref_buckets, uint32_t* out, hipStream_t st);
hipError_t smem_launch_occ192(const uint32_t* occ64, uint64_t n_blocks, uint32_t* out, hipStream_t st);
// the bi-intervals of every string of 1..k bases (k <= 15): table L at entry
// (4^L - 4) / 3, index = the string's 2-bit codes, first base highest; 16-B
// packed entries (x0, x1, x2 low words, bits 32-33 in word 3), x2 = 0 when absent
hipError_t smem_launch_kmer_table(const uint32_t* occ64, uint64_t primary, const uint64_t* L2, int k, uint4* kt,
                                  hipStream_t st);
// mn[L] = the smallest x2 of table level L, L = 1..k (mn: k + 1 device words)
hipError_t smem_launch_kmer_min(const uint4* kt, int k, unsigned long long* mn, hipStream_t st);
// *mn_next = the smallest size among the strings of k + 1 bases (0: one is absent), computed from level k
// and the index without storing the level (k <= 14; one device word).  *not_strict (may be null; one device
// word) = 1 if a present string of k bases has a one-base extension as large as itself, else 0
hipError_t smem_launch_kmer_min_next(const uint32_t* occ64, uint64_t primary, const uint64_t* L2, const uint4* kt, int k,
                                     unsigned long long* mn_next, unsigned long long* not_strict, hipStream_t st);
hipError_t smem_launch_finalize(const smem::FinalizeParams* F, int write, hipStream_t st);
hipError_t smem_launch_fill_i32(int32_t* p, int32_t v, int n, hipStream_t st);
hipError_t smem_launch_pack_intv(const smem::Intv* in, uint64_t n, uint4* out, hipStream_t st);
hipError_t smem_launch_ovf_slot(const int32_t* items, int n_ovf, int32_t* ovf_slot, hipStream_t st);
hipError_t smem_launch_sa_count(const smem::SaParams* S, hipStream_t st);
hipError_t smem_launch_sa_densify(const smem::SaParams* S, uint32_t dshift, uint64_t n_dense, uint64_t* dense,
                                  hipStream_t st);
// the same dense[] by hop + chase passes (link: n_dense words of scratch; n_dense < 2^32;
// max_blocks != 0 caps the lane-strided grids, leaving CUs to other work)
hipError_t smem_launch_sa_densify2(const smem::SaParams* S, uint32_t dshift, uint64_t n_dense, uint64_t* link,
                                   uint64_t* dense, unsigned max_blocks, hipStream_t st);
hipError_t smem_launch_sa_walk(const smem::SaParams* S, int grid, hipStream_t st);
hipError_t smem_launch_offsets(const uint64_t* in, uint64_t* out, int n, void* temp, size_t* temp_bytes,
                               hipStream_t st);
// the same over in[0], in[stride], ...; total != nullptr also receives out[n]
hipError_t smem_launch_offsets_strided(const uint64_t* in, int stride, uint64_t* out, int n, void* temp,
                                       size_t* temp_bytes, uint64_t* total, hipStream_t st);
}
