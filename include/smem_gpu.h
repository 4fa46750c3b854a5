/*
 * smem_gpu.h — C ABI of the MI355X SMEM seeding engine (libsmemgpu.so).
 *
 * Drop-in boundary for BWA-MEM's seeding loop.  In the
 * reference, every kt_for_batch worker (software/kthread_batch.c:29-59)
 * runs mem_chain_batched -> mem_insert_seed_batched -> smem_next2_batched ->
 * bwt_smem1_batched (software/bwamem.c:542-591,357-451,110-241,
 * software/bwt.c:444-774), which packs <=128 reads per FPGA hand-shake
 * through the HARP manager thread (software/fastmap.c:320-429) and the AAL
 * glue (software/HelloALINLB.cpp:254-485).  This library replaces that whole
 * chain: one call seeds a batch of reads on the GPU and returns, per read,
 * exactly the sequence of interval lists smem_next2() (software/bwamem.c:244)
 * returns under mem_insert_seed() (software/bwamem.c:453-460) — bit-exact,
 * in order — so the caller's chaining body (software/bwamem.c:462-499) runs
 * unchanged.
 *
 * Plain C types only.  All entry points return 0 (SMEM_OK) or a negative
 * SMEM_E_* code; on a negative code the caller may fall back to its own CPU
 * path, mirroring the reference's reject -> CPU semantics
 * (software/bwt.c:686-717).  No entry point silently computes on the CPU.
 *
 * Failure contract: every entry point that runs work on a device returns
 * only once all of that work has finished or been abandoned (its streams
 * are synchronised on every return path), so no copy of the call lands in
 * host memory after the caller has resumed, whatever the code.  A HIP
 * runtime failure (SMEM_E_DEVICE) marks the device faulted: every later
 * call on it returns SMEM_E_DEVICE at once without enqueuing anything, so a
 * caller that takes its CPU path on SMEM_E_DEVICE computes exactly what the
 * reference computes.  Allocation failures are SMEM_E_NOMEM and leave the
 * device usable.  SMEM_GPU_FAIL=<stage>:<k>[:sticky] (stage: upload, seed,
 * sa, chain, aln, fin, g2a, sam, matesw, pair, fetch, any) injects SMEM_E_DEVICE into every k-th
 * call of the stage after its work is enqueued, to test that contract.
 */
#ifndef SMEM_GPU_H
#define SMEM_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMEM_OK           0
#define SMEM_E_ARG       -1   /* bad argument / shape */
#define SMEM_E_NOMEM     -2   /* host or device allocation failed */
#define SMEM_E_IO        -3   /* file I/O */
#define SMEM_E_DEVICE    -4   /* no usable HIP device or a HIP runtime error */
#define SMEM_E_INTERNAL  -5
#define SMEM_E_CAPACITY  -6   /* batch larger than the capacity it was created with */

/* bi-interval; identical layout to bwtintv_t (software/bwt.h:60-62):
 * x[0] forward SA start, x[1] reverse-complement SA start, x[2] size,
 * info = (query begin << 32) | query end (end exclusive). */
typedef struct { uint64_t x[3], info; } smem_intv_t;

/* FM-index in host memory.  The leading fields follow bwt_t
 * (software/bwt.h:46-51): primary, L2[5], seq_len, bwt_size, bwt. */
typedef struct {
	uint64_t primary;     /* S^-1(0): BWT row of the $ suffix */
	uint64_t L2[5];       /* cumulative base counts, L2[0] = 0 */
	uint64_t seq_len;     /* = L2[4] */
	uint64_t bwt_size;    /* number of uint32 words (Occ checkpoints interleaved) */
	uint32_t *bwt;        /* interleaved BWT + Occ, software/bwtindex.c:128-150 layout */
	int owns;             /* bwt was allocated by this library */
} smem_index_t;

/* Sampled suffix array for bwt_sa (software/bwt.c:80-114): sa[r] =
 * SA[r * sa_intv] for r < n_sa = (seq_len + sa_intv) / sa_intv, sa[0] =
 * (uint64_t)-1 as bwt_cal_sa leaves it.  primary / L2 / seq_len are those of
 * the .bwt it belongs to (the .sa header, software/bwt.c:852-863).  sa holds
 * n_sa + 1 words (one zero pad). */
typedef struct {
	uint64_t primary;
	uint64_t L2[5];
	uint64_t seq_len;
	uint64_t sa_intv;
	uint64_t n_sa;
	uint64_t *sa;
	int owns;
} smem_sa_t;

/* the mem_opt_t fields the seeding loop reads (software/bwamem.h:44-48,
 * software/bwamem.c:456-458) */
typedef struct {
	int min_seed_len;     /* -k, default 19 */
	float split_factor;   /* -r, default 1.5 */
	int split_width;      /* -s, default 10 */
	int start_width;      /* 1, or 2 when MEM_F_NO_EXACT (-e) */
} smem_opt_t;

typedef struct smem_gpu smem_gpu_t;       /* one device + its resident index */
typedef struct smem_batch smem_batch_t;   /* one worker's reads / results / scratch on one device */

/* defaults of mem_opt_init() (software/bwamem.c:58-65) */
void smem_opt_default(smem_opt_t *opt);

/* ---------------------------------------------------------------- index */
/* Build the .bwt of genome codes (0..3, forward strand only; the reverse
 * complement is appended as bns_fasta2bntseq(for_only=0) does).  Output is
 * byte-identical to `bwa index -a is` (software/bwtindex.c:187). */
int  smem_bwt_build(const uint8_t *fwd_codes, uint64_t n_fwd, smem_index_t *idx);
/* Same .bwt, built on a HIP device by prefix doubling + radix sort
 * (seconds for Gbp genomes); 2 x n_fwd must stay below 2^32 - 1. */
int  smem_bwt_build_gpu(int device, const uint8_t *fwd_codes, uint64_t n_fwd, smem_index_t *idx);
/* .bwt file I/O (software/bwt.c:841-850, 899-918) */
int  smem_bwt_read(const char *fn, smem_index_t *idx);
int  smem_bwt_write(const char *fn, const smem_index_t *idx);
void smem_index_free(smem_index_t *idx);
/* smem_bwt_build + the sampled SA bwa index writes beside it (`bwa index`
 * .sa, sa_intv = 32 there, software/bwtindex.c:280); sa_intv a power of 2 */
int  smem_bwt_build_sa(const uint8_t *fwd_codes, uint64_t n_fwd, int sa_intv, smem_index_t *idx, smem_sa_t *sa);
/* the same on a HIP device (prefix doubling, as smem_bwt_build_gpu) */
int  smem_bwt_build_gpu_sa(int device, const uint8_t *fwd_codes, uint64_t n_fwd, int sa_intv, smem_index_t *idx,
                           smem_sa_t *sa);
/* The bucketed builder with 64-bit suffix positions (both strands up to 2^34
 * symbols: a human-size genome).  smem_bwt_build_gpu(_sa) switch to it by
 * themselves once 2 * n_fwd no longer fits 32 bits; called directly it runs
 * at any size (tests compare it with the CPU builder).  sa may be NULL. */
int  smem_bwt_build_gpu_large(int device, const uint8_t *fwd_codes, uint64_t n_fwd, int sa_intv, smem_index_t *idx,
                              smem_sa_t *sa);
/* .sa file I/O (software/bwt.c:852-897) */
int  smem_sa_read(const char *fn, smem_sa_t *sa);
int  smem_sa_write(const char *fn, const smem_sa_t *sa);
void smem_sa_free(smem_sa_t *sa);

/* --------------------------------------------------------------- device */
/* Number of visible HIP devices (0 on a machine without a GPU). */
int  smem_gpu_device_count(void);

/* Upload the index to `device` and keep it resident in HBM.  Replaces the
 * FPGA index upload in bwa_idx_load_bwt (software/bwa.c:286-307) and the
 * AAL buffer setup (software/HelloALINLB.cpp:344-451).  The words are copied;
 * the caller's arrays may be freed afterwards.  Limits: seq_len < 2^34 and
 * an index below 4 GiB (both strands of ~8.5 Gbp); SMEM_E_ARG otherwise. */
int  smem_gpu_init(smem_gpu_t **gpu, int device, const uint32_t *bwt, uint64_t bwt_size,
                   uint64_t primary, const uint64_t L2[5]);
void smem_gpu_shutdown(smem_gpu_t *gpu);

/* Multi-GPU: the index replicated on `n` devices, one smem_gpu_t each
 * (reads shard across GPUs, no collective).  devices[i] (NULL:
 * 0 .. n-1) may repeat a device (two contexts on one GPU).  sa / pac (NULL:
 * none) are made resident as smem_gpu_load_sa / smem_gpu_load_pac do.  The
 * uploads run side by side, one host thread per device.  Replaces, for all
 * devices at once, the single FPGA upload of software/bwa.c:286-307.  On
 * failure every device opened so far is shut down and gpus[] is zeroed. */
int  smem_gpu_init_devices(smem_gpu_t **gpus, int n, const int *devices, const uint32_t *bwt, uint64_t bwt_size,
                           uint64_t primary, const uint64_t L2[5], const smem_sa_t *sa, const uint8_t *pac,
                           int64_t l_pac);
/* The same with the device work on one host thread per device: the call
 * checks its arguments and returns; the uploads (and the .sa densification)
 * run while the caller goes on (bwa mem reads its first chunk).  Every entry
 * point that touches a device waits for its upload first; smem_gpu_wait_ready
 * waits explicitly.  A failed upload faults the handle (smem_gpu_fault 3):
 * every call on it is refused with SMEM_E_DEVICE, the caller's CPU path.  bwt,
 * sa->sa and pac must stay valid until the device is ready (the smem_sa_t
 * itself is copied). */
int  smem_gpu_init_devices_async(smem_gpu_t **gpus, int n, const int *devices, const uint32_t *bwt, uint64_t bwt_size,
                                 uint64_t primary, const uint64_t L2[5], const smem_sa_t *sa, const uint8_t *pac,
                                 int64_t l_pac);
/* Waits until everything the device does in the background has finished:
 * the upload chain, the .sa densification and any smem_gpu_reserve_slots
 * sizing (batches need not wait: their SA lookups use the uploaded samples
 * until the densification is done). */
int  smem_gpu_wait_ready(smem_gpu_t *gpu);
/* The steps of smem_gpu_init_devices_async one by one, so that each starts
 * as soon as its input is in memory (bwa_idx_load reads .bwt, then .sa, then
 * .pac): open_async checks the device and uploads the index in the
 * background; load_sa_async / load_pac_async queue behind it.  Same waiting
 * and fault rules. */
int  smem_gpu_open_async(smem_gpu_t **gpu, int device, const uint32_t *bwt, uint64_t bwt_size, uint64_t primary,
                         const uint64_t L2[5]);
int  smem_gpu_load_sa_async(smem_gpu_t *gpu, const smem_sa_t *sa);
int  smem_gpu_load_pac_async(smem_gpu_t *gpu, const uint8_t *pac, int64_t l_pac);
/* "0,2,5" -> devices[] = {0, 2, 5}; NULL or "" -> every visible device.
 * Returns the count, or a negative code (bad list, more than max_devices,
 * no device for the empty spec). */
int  smem_gpu_parse_devices(const char *spec, int *devices, int max_devices);

/* ------------------------------------------------------------ one shot */
/* Thread-safe; may be called concurrently from kt_for_batch workers (each
 * calling thread gets its own buffers, created on first use and freed by
 * smem_gpu_shutdown; the streams come from the device's admission pool, see
 * smem_gpu_set_max_active).  seq[i] are nt4 codes (0..3, >3 ambiguous),
 * len[i] their lengths; the results stay valid until the same thread calls
 * smem_gpu_collect again.  Read them with smem_batch_read(*batch_out, i, ...). */
int  smem_gpu_collect(smem_gpu_t *gpu, int n_reads, const uint8_t *const *seq, const int *len,
                      const smem_opt_t *opt, smem_batch_t **batch_out);
/* The same with the batch chosen by worker slot (slot >= 0: the kt_for_batch
 * tid of software/kthread_batch.c:38, which the reference maps to its
 * per-worker FPGA buffer through get_thread_id, software/bwt.c:51-58; the slot's
 * batch is reused by whichever thread holds the slot next, so the short-lived
 * threads bwa mem starts per chunk do not each leave a batch behind; two
 * threads must not use one slot at once; slot < 0: the calling thread's batch,
 * as smem_gpu_collect).  flags: SMEM_COLLECT_NO_FETCH -- results stay in HBM
 * for smem_batch_sa / _chain / _chain2aln, and smem_batch_fetch_mask copies
 * only what the caller reads. */
#define SMEM_COLLECT_NO_FETCH 1
int  smem_gpu_collect_ex(smem_gpu_t *gpu, int slot, int n_reads, const uint8_t *const *seq, const int *len,
                         const smem_opt_t *opt, int flags, smem_batch_t **batch_out);
/* Pre-size worker slots [0, n_slots) of smem_gpu_collect_ex for batches of up
 * to reads_per_slot reads of up to max_len bases, with the later stages'
 * scratch and pinned result buffers sized at generous per-read estimates, and
 * load the code object of every kernel file (hipFuncGetAttributes: a kernel's
 * code object otherwise loads on its first launch); SMEM_GPU_WARMUP=full runs
 * one warm-up pass of every stage over a few reads cut from the resident .pac
 * instead.  Replaces the
 * per-worker buffers main_mem allocates before the first chunk
 * (software/fastmap.c:207-210).  Runs on a background host thread: the call
 * returns at once, and the first smem_gpu_collect* on the device waits for it.
 * A batch larger than reserved is re-created on first use, as without it. */
int  smem_gpu_reserve_slots(smem_gpu_t *gpu, int n_slots, int reads_per_slot, int max_len);
/* Reads one seeding launch holds in flight on the device at once: the
 * persistent grid's read owners (CUs x lanes per CU x owners per wave / 64;
 * 92,160 for the default kernel on MI355X).  A worker batch of at least this
 * many reads fills the device by itself (the binding's batch plan).
 * Needs no open device work: the CU count comes from the device's attributes. */
int  smem_gpu_grid_reads(const smem_gpu_t *gpu);
/* The device's compute units, by which the stages size their grids (mate
 * rescue's wave kernel: MSW_WAVES_PER_CU waves each, csrc/matesw_kernels.h);
 * < 0 on error. */
int  smem_gpu_cu_count(const smem_gpu_t *gpu);
/* Admission, the HARP manager's role (software/fastmap.c:320-429): at most n
 * calls run work on the device at once, each on one of n leased stream pairs
 * (a device carries at most 2n streams however many workers share it); the
 * others wait for a pair instead of being rejected.  Default 8, or
 * SMEM_GPU_MAX_ACTIVE at smem_gpu_init; 0 restores the default. */
int  smem_gpu_set_max_active(smem_gpu_t *gpu, int n);
/* The admission limit in force (what smem_gpu_set_max_active / SMEM_GPU_MAX_ACTIVE
 * set): the batches a device runs at once, for a caller's batch plan. */
int  smem_gpu_get_max_active(const smem_gpu_t *gpu);
/* 0: the device has not faulted; 1: a HIP runtime failure faulted it (the
 * HIP runtime may also have printed its own diagnostics -- on a queue abort,
 * a dump of the queue's packets on stdout); 2: an injected sticky fault
 * (SMEM_GPU_FAIL); 3: smem_gpu_init_devices_async could not upload the index
 * (a refusal, e.g. an allocation that does not fit; an upload that failed on a
 * HIP runtime error reports 1).  msg (may be NULL) gets the first failure's text. */
int  smem_gpu_fault(const smem_gpu_t *gpu, char *msg, int msg_len);
/* Memory held: a batch's device and pinned host buffers (they grow to the
 * largest batch seen); a device's resident index (Occ64, densified SA and the
 * uploaded samples, .pac) and the batches it keeps (worker slots, per-thread
 * batches, the streaming pool) -- what a maintainer sizes -t / -b against. */
int  smem_batch_memory(const smem_batch_t *b, uint64_t *device_bytes, uint64_t *pinned_bytes);
int  smem_gpu_memory(smem_gpu_t *gpu, uint64_t *index_bytes, uint64_t *batch_bytes, uint64_t *pinned_bytes,
                     int *n_batches);

/* ------------------------------------------------------------ streaming */
/* bwa mem's chunk loop (software/fastmap.c:213-228, mem_process_seqs ->
 * kt_for_batch, software/bwamem.c:1614-1640, software/kthread_batch.c:29-59)
 * over one device, for read sets larger than one batch.  Reads [0, n_reads)
 * (nt4 codes, offs[n_reads + 1] into codes) are cut into chunks of at most
 * chunk_reads; n_workers host threads each own a batch (pinned staging
 * buffers, a HIP stream, device buffers) and run whole chunks: stage + H2D,
 * seeding + compaction, D2H into pinned host memory, then fn(ctx, chunk,
 * first_read, n, batch) on that worker's thread, where smem_batch_read /
 * smem_batch_results give the chunk's results (valid until fn returns).
 * Chunks are claimed in order; callbacks of different workers may overlap
 * and complete out of order (the chunk index orders them).  flags:
 * SMEM_STREAM_PAIRS -- n_reads must be even and chunk boundaries are kept
 * even, so both mates of a pair (reads 2k, 2k+1, interleaved as
 * software/bwamem.c:1600-1609 reads them) land in one chunk;
 * SMEM_STREAM_PACKED -- each interval crosses PCIe as a 16-B smem_pintv_t
 * (reads < 8192 bp), read with smem_batch_results_packed + smem_pintv_unpack
 * in the callback; SMEM_STREAM_RELEASE -- free the workers' batches when the
 * call returns.  Otherwise the handle keeps at most n_workers of them for
 * the next call (each holds ~1 GB of pinned host memory per 1M-read chunk;
 * a later call with fewer workers shrinks the pool, smem_gpu_shutdown frees
 * it).  fn may be NULL; a non-zero return from fn stops the stream and is
 * returned. */
typedef int (*smem_chunk_fn)(void *ctx, int64_t chunk, int64_t first_read, int n_reads, const smem_batch_t *b);
#define SMEM_STREAM_PAIRS   1   /* interleaved mates: chunks keep pairs whole */
/* (a call with a read longer than SMEM_PINTV_MAX_LEN = 8191 bp is refused with SMEM_E_ARG before any
 * chunk runs; the test suite covers packed reads of 8191 bp, and 8192 bp for the refusal) */
#define SMEM_STREAM_PACKED  2   /* results as 16-B smem_pintv_t (smem_batch_results_packed): half the D2H */
#define SMEM_STREAM_RELEASE 4   /* do not keep the workers' batches (pinned buffers) for the next call */
typedef struct {
	double wall_s;           /* first chunk claimed -> last chunk delivered */
	uint64_t n_reads, n_chunks, n_intv;
	uint64_t h2d_bytes;      /* reads + offsets copied host -> device */
	uint64_t d2h_bytes;      /* intervals + list sizes + offsets copied device -> host */
	int workers;
	double stage_s, run_s, fetch_s;  /* summed over chunks: staging + H2D issue, smem_batch_run, smem_batch_fetch */
} smem_stream_stats_t;
int  smem_gpu_seed_stream(smem_gpu_t *gpu, int64_t n_reads, const uint8_t *codes, const uint64_t *offs,
                          const smem_opt_t *opt, int chunk_reads, int n_workers, int flags, smem_chunk_fn fn,
                          void *ctx, smem_stream_stats_t *stats);

/* ------------------------------------------------------- batch (explicit) */
/* max_len: the longest read the batch will hold, 1 .. 2^24 (more is
 * SMEM_E_ARG).  It sets the per-read output capacity (max_len / 2 + 32
 * intervals; a read with more goes through the overflow pass) and the list
 * arenas (max_len + 2 entries).  The test suite covers reads of 0 bp to
 * 70,698 bp through seeding, smem_batch_sa and smem_batch_chain
 * (tests/test_gpu_long_reads.py); nothing longer has been run. */
int  smem_batch_create(smem_gpu_t *gpu, int max_reads, uint64_t max_bases, int max_len, smem_batch_t **b);
void smem_batch_destroy(smem_batch_t *b);
/* stage reads: per-read pointers (bseq1_t style) or one concatenated array
 * with offsets[n_reads+1]; copied host -> device on the batch stream */
int  smem_batch_set_reads(smem_batch_t *b, int n_reads, const uint8_t *const *seq, const int *len);
int  smem_batch_set_reads_packed(smem_batch_t *b, int n_reads, const uint8_t *codes, const uint64_t *offsets);
/* run the seeding loop on the resident reads; results stay in HBM */
int  smem_batch_run(smem_batch_t *b, const smem_opt_t *opt);
/* copy results device -> host (pinned): every stage that has run */
int  smem_batch_fetch(smem_batch_t *b);
/* copy only the named outputs: the interval lists (smem_batch_read /
 * _results), the SA positions (smem_batch_sa_results), the chains and seeds
 * (smem_batch_chain_results), the regions (smem_batch_aln_results).  Naming a
 * stage that has not run on this batch is SMEM_E_ARG.  A view whose output was
 * not copied by the last fetch returns SMEM_E_ARG. */
#define SMEM_FETCH_INTV    1
#define SMEM_FETCH_SA      2
#define SMEM_FETCH_CHAINS  4
#define SMEM_FETCH_REGS    8
#define SMEM_FETCH_ALL    15
#define SMEM_FETCH_FIN    16   /* smem_batch_reg_finalize's results (smem_batch_fin_results); not part of ALL */
#define SMEM_FETCH_ALN    32   /* smem_batch_reg2aln's results (smem_batch_aln2_results); not part of ALL */
#define SMEM_FETCH_SAM    64   /* smem_batch_sam's text (smem_batch_sam_results); not part of ALL */
int  smem_batch_fetch_mask(smem_batch_t *b, int mask);
/* per-read view of fetched results: the concatenation of all smem_next2
 * lists in order (n_intv intervals) and the size of each list (n_calls) */
int  smem_batch_read(const smem_batch_t *b, int i, const smem_intv_t **intv, int *n_intv,
                     const uint32_t **call_n, int *n_calls);
/* whole-batch views of fetched results: intv_off/call_off have n_reads+1 entries */
int  smem_batch_results(const smem_batch_t *b, const smem_intv_t **intv, const uint64_t **intv_off,
                        const uint32_t **call_n, const uint64_t **call_off);

/* 16-B wire form of a bwtintv_t (SMEM_STREAM_PACKED): x0, x1, x2 low words;
 * w = x0 bits 32-33 | x1 bits 32-33 << 2 | x2 bits 32-33 << 4 | query begin << 6
 * | query end << 19 (13 bits each) */
typedef struct { uint32_t x0, x1, x2, w; } smem_pintv_t;
#define SMEM_PINTV_MAX_LEN 8191
static inline void smem_pintv_unpack(const smem_pintv_t *p, smem_intv_t *o)
{
	o->x[0] = (uint64_t)(p->w & 3) << 32 | p->x0;
	o->x[1] = (uint64_t)(p->w >> 2 & 3) << 32 | p->x1;
	o->x[2] = (uint64_t)(p->w >> 4 & 3) << 32 | p->x2;
	o->info = (uint64_t)(p->w >> 6 & 8191) << 32 | (p->w >> 19);
}
/* the packed view of a batch fetched in SMEM_STREAM_PACKED mode */
int  smem_batch_results_packed(const smem_batch_t *b, const smem_pintv_t **pintv, const uint64_t **intv_off,
                               const uint32_t **call_n, const uint64_t **call_off);

/* ------------------------------------------------------- SA lookup */
/* Keep the sampled SA of the uploaded index resident in HBM (the index's
 * .sa, software/bwt.c:877-897; bwa_idx_load's bwt_restore_sa).  SMEM_E_ARG
 * if it does not belong to the index.  Reads sa->sa[0 .. n_sa-1] only (the
 * reference's bwt->sa array as is).  The device copy is densified to every
 * 4th row by LF walks from these samples (8 B per 4 symbols of HBM); lookups
 * return exactly what bwt_sa does with the .sa's own interval.  The
 * densification runs in the background (~0.3 s at human size): the call
 * returns after the upload, and until the densification has finished
 * smem_batch_sa walks to the uploaded samples instead (the same positions,
 * more LF steps), so no batch waits for it (SMEM_GPU_SYNC_INIT=1: wait here;
 * SMEM_GPU_SA_RAW=1: always the uploaded samples).  The uploaded samples stay
 * resident beside the dense copy until smem_gpu_shutdown. */
int  smem_gpu_load_sa(smem_gpu_t *gpu, const smem_sa_t *sa);
/* After smem_batch_run: bwt_sa (software/bwt.c:104-114) of every seed
 * occurrence mem_insert_seed() generates from the lists — each interval with
 * seed length >= min_seed_len and x2 <= max_occ, rows x0 .. x0+x2-1
 * (software/bwamem.c:462-474) — on the GPU.  smem_batch_fetch then copies
 * them; smem_batch_sa_results gives the positions (forward-reverse
 * coordinates, the mem_seed_t rbeg) in interval order and occ_off[n_intv + 1]
 * indexed by flat interval (the numbering of smem_batch_results). */
int  smem_batch_sa(smem_batch_t *b, int min_seed_len, int max_occ);
int  smem_batch_sa_results(const smem_batch_t *b, const uint64_t **pos, const uint64_t **occ_off, uint64_t *n_occ);

/* ------------------------------------------------------- chaining */
/* mem_seed_t (software/bwamem.c:317-320) */
typedef struct {
	int64_t rbeg;          /* forward-reverse coordinate (bwt_sa) */
	int32_t qbeg, len;
} smem_seed_t;
/* one chain of mem_chain_t (software/bwamem.c:322-326): pos and its n seeds,
 * seeds[seed_off .. seed_off + n) of smem_batch_chain_results */
typedef struct {
	int64_t pos;
	uint64_t seed_off;
	int32_t n, pad;
} smem_chain_t;
/* the mem_opt_t fields chaining reads (software/bwamem.h:39-53) */
typedef struct {
	int w;                    /* band width, 100 */
	int max_chain_gap;        /* 10000 */
	float mask_level;         /* 0.50 */
	float chain_drop_ratio;   /* 0.50 */
	int filter;               /* 1: mem_chain_flt after mem_chain, as mem_align1_core does */
} smem_chain_opt_t;
void smem_chain_opt_default(smem_chain_opt_t *opt);
/* After smem_batch_sa: mem_chain (software/bwamem.c:593-614) of every read on
 * the GPU — the seed sequence of mem_insert_seed (software/bwamem.c:462-499),
 * test_and_merge into the kbtree of chains, in-order chain list — and, when
 * opt->filter, mem_chain_flt (software/bwamem.c:629-690).  l_pac is the
 * forward strand length (bns->l_pac).  The filter's drop margin uses the
 * min_seed_len given to smem_batch_sa.  smem_batch_fetch copies the chains;
 * smem_batch_chain_results returns them per read: chain_off[n_reads + 1]
 * into chains[], each chain's seeds contiguous in seeds[]. */
int  smem_batch_chain(smem_batch_t *b, int64_t l_pac, const smem_chain_opt_t *opt);
int  smem_batch_chain_results(const smem_batch_t *b, const smem_chain_t **chains, const uint64_t **chain_off,
                              const smem_seed_t **seeds, uint64_t *n_chains, uint64_t *n_seeds);

/* --------------------------------------------------- SW extension */
/* one ksw_extend2 call (software/ksw.c:379) as mem_chain2aln makes it
 * (software/bwamem.c:1136, 1164): query / target are offsets into the code
 * pools (0..4; the left extension's reversed sequences as the caller builds
 * them), m = 5 */
typedef struct {
	uint64_t q_off, t_off;
	int32_t qlen, tlen;       /* 1 <= qlen <= 255, tlen >= 0 */
	int32_t w, end_bonus, zdrop, h0;
} smem_ksw_task_t;
/* the return value and the five out-parameters of ksw_extend2 */
typedef struct {
	int32_t score, qle, tle, gtle, gscore, max_off;
} smem_ksw_result_t;
typedef struct {
	int8_t mat[25], pad[3];   /* bwa_fill_scmat (software/bwa.c:84-93) */
	int32_t o_del, e_del, o_ins, e_ins;
} smem_ksw_opt_t;
/* mem_opt_init's scoring (software/bwamem.c:50-52): a 1, b 4, gaps 6 + 1 */
void smem_ksw_opt_default(smem_ksw_opt_t *opt);
/* ksw_extend2 of every task on the GPU, results in task order: the same
 * values the reference returns.  Host buffers in and out; kernel_ms (may be
 * NULL) gets the kernel's HIP-event time.  SMEM_E_ARG for a task outside the
 * limits above or gap penalties with e < 1 or o < 0 (the caller extends
 * those on the CPU, as the reference's reject path would). */
int  smem_ksw_extend(smem_gpu_t *gpu, int n, const smem_ksw_task_t *tasks, const uint8_t *q, uint64_t q_bytes,
                     const uint8_t *t, uint64_t t_bytes, const smem_ksw_opt_t *opt, smem_ksw_result_t *out,
                     double *kernel_ms);

/* one ksw_align2 call (software/ksw.c:342) as mem_chain2aln_short makes it
 * (software/bwamem.c:835-836): xtra = KSW_XSUBO | KSW_XSTART | (KSW_XBYTE when
 * qlen * a < 250) | min_seed_len * a; query / target offsets into code pools */
typedef struct {
	uint64_t q_off, t_off;
	int32_t qlen, tlen;       /* 1 <= qlen <= 256, 0 <= tlen <= 256 */
	int32_t xtra, pad;        /* KSW_XBYTE 0x10000, KSW_XSTOP 0x20000, KSW_XSUBO 0x40000, KSW_XSTART 0x80000 */
} smem_ksw_atask_t;
/* kswr_t (software/ksw.h:13-15) */
typedef struct {
	int32_t score, te, qe, score2, te2, tb, qb;
} smem_ksw_aresult_t;
/* ksw_align2 (striped local SW: ksw_u8 with KSW_XBYTE, else ksw_i16; the start
 * pass with KSW_XSTART) of every task on the GPU, one wave per problem: the
 * kswr_t the reference returns.  The device routine is the one
 * smem_chain2aln / smem_batch_chain2aln run for mem_chain2aln_short. */
int  smem_ksw_align2(smem_gpu_t *gpu, int n, const smem_ksw_atask_t *tasks, const uint8_t *q, uint64_t q_bytes,
                     const uint8_t *t, uint64_t t_bytes, const smem_ksw_opt_t *opt, smem_ksw_aresult_t *out,
                     double *kernel_ms);
/* The same call for the targets mem_matesw builds (software/bwamem_pair.c:144: a window of
 * several hundred to a few thousand reference bases): 1 <= qlen <= 256, 0 <= tlen <=
 * SMEM_KSWA_MAX_TLEN, anything else SMEM_E_ARG before any device work.  One wave per problem;
 * the target is fetched 64 rows at a time and the suboptimal list, up to tlen / 2 + 1 entries,
 * is kept in LDS (8200 B a wave).  Every kswr_t field is the reference's. */
#define SMEM_KSWA_MAX_TLEN 2048
int  smem_ksw_align2_long(smem_gpu_t *gpu, int n, const smem_ksw_atask_t *tasks, const uint8_t *q, uint64_t q_bytes,
                          const uint8_t *t, uint64_t t_bytes, const smem_ksw_opt_t *opt, smem_ksw_aresult_t *out,
                          double *kernel_ms);

/* ------------------------------------------- chains -> alignment regions */
/* mem_alnreg_t (software/bwamem.h:62-74); hash / sub / sub_n / secondary are
 * left 0 here, as mem_chain2aln leaves them (mem_mark_primary sets them later) */
typedef struct {
	int64_t rb, re;
	int32_t qb, qe, score, truesc, sub, csub, sub_n, w, seedcov, secondary;
	uint64_t hash;
} smem_alnreg_t;
/* the mem_opt_t fields mem_chain2aln reads (software/bwamem.h:33-45) */
typedef struct {
	smem_ksw_opt_t sc;        /* matrix and gap penalties */
	int a;                    /* match score, 1 */
	int w;                    /* band width, 100 */
	int zdrop;                /* 100 */
	int pen_clip5, pen_clip3; /* 5, 5 */
	int min_seed_len;         /* 19 */
} smem_aln_opt_t;
void smem_aln_opt_default(smem_aln_opt_t *opt);
/* The loop of mem_align1_core over every read's chains (software/bwamem.c:1452-1460):
 * mem_chain2aln_short, then mem_chain2aln when it declines (software/bwamem.c:805-852,
 * 1040-1188), on the GPU, one wave per read.  Replaces the host-side calls at
 * software/bwamem.c:1421-1422 / 1457-1458.  Inputs are host buffers in the layout
 * smem_batch_chain_results returns (chains[chain_off[r] .. chain_off[r+1]) of read r,
 * seeds[n_seeds] indexed by smem_chain_t.seed_off) plus the reads (nt4 codes, offs[n+1])
 * and the 2-bit forward-strand .pac (software/bntseq.c:303-309, l_pac bases).
 * regs must hold one region per chain seed (sum of chains' n); reg_off[n_reads + 1]
 * gets each read's regions, in the order the reference appends them.  Reads longer
 * than 1024 bp give SMEM_E_ARG. */
int  smem_chain2aln(smem_gpu_t *gpu, int n_reads, const uint8_t *codes, const uint64_t *offs,
                    const smem_chain_t *chains, const uint64_t *chain_off, const smem_seed_t *seeds, uint64_t n_seeds,
                    const uint8_t *pac, int64_t l_pac, const smem_aln_opt_t *opt, smem_alnreg_t *regs,
                    uint64_t *reg_off, double *kernel_ms);
/* (pac may be NULL when smem_gpu_load_pac made this l_pac's .pac resident.
 * Query codes must be 0..4 and no two chains may share seeds: SMEM_E_ARG.) */

/* Keep the 2-bit forward-strand .pac of the uploaded index resident in HBM
 * (bwa_idx_load's idx->pac, software/bwa.c:325-330); 2 * l_pac must equal the
 * index's seq_len.  Replacing a loaded .pac must not overlap a chains ->
 * regions call (smem_batch_chain2aln, smem_chain2aln) on the same handle:
 * such a call may still read the old copy. */
int  smem_gpu_load_pac(smem_gpu_t *gpu, const uint8_t *pac, int64_t l_pac);
/* Device-resident twin of smem_chain2aln: after smem_batch_chain (filter = 1,
 * as mem_align1_core_batched filters before extending, software/bwamem.c:1414-1422),
 * mem_chain2aln_short / mem_chain2aln of every chain of every read of the batch
 * over the reads, chains and seeds still in HBM and the resident .pac: no host
 * round trip, no per-call allocation once the batch has grown.  smem_batch_fetch
 * copies the regions; smem_batch_aln_results returns them with reg_off[n_reads + 1]. */
int  smem_batch_chain2aln(smem_batch_t *b, const smem_aln_opt_t *opt);
int  smem_batch_aln_results(const smem_batch_t *b, const smem_alnreg_t **regs, const uint64_t **reg_off,
                            uint64_t *n_regs);

/* ------------------------------------------- regions -> alignments */
#define SMEM_ALN_UNMAPPED 1
#define SMEM_ALN_NOCIGAR  2
#define SMEM_ALN_REJECT   3
#define SMEM_ALN_XREF     4   /* smem_batch_reg2aln with a contig table only: the region bridges a contig
                                 boundary (the test at the head of bwa_fix_xref2, software/bwa.c:195-199);
                                 no alignment, the caller does it on the CPU */
/* what mem_reg2aln (software/bwamem.c:1481-1553) makes of one region, short of
 * the contig lookup, MAPQ and flags */
typedef struct {
	int64_t  pos;        /* 0-based forward-strand coordinate in the concatenated .pac (bns_depos of
	                        rb, or of re-1 on the reverse strand), after a leading deletion was squeezed out;
	                        -1 when status != 0 */
	int32_t  is_rev, n_cigar, NM, score;   /* score: ksw_global2's of the last try */
	int32_t  tries;      /* 1..3 bwa_gen_cigar2 calls made (the band-doubling loop) */
	int32_t  status;     /* 0 ok; SMEM_ALN_UNMAPPED (rb<0 or re<0); SMEM_ALN_NOCIGAR (bwa_gen_cigar2
	                        returned 0: empty, or bridging l_pac; NM -1, tries 1); SMEM_ALN_REJECT (outside
	                        the limits below: the caller does it on the CPU, the reference's reject -> CPU
	                        convention) */
	uint64_t cigar_off;  /* into cigar[]: n_cigar words, len<<4|op, op 0 M 1 I 2 D 3 S (clips as mem_reg2aln adds them) */
	uint64_t md_off; int32_t md_len, pad;  /* into md[]: the MD string, no terminator */
} smem_aln_t;
/* The alignment part of mem_reg2aln for every region of every read, on the GPU:
 * the band from infer_bw (software/bwamem.c:1194-1201, 1504-1508), up to three
 * bwa_gen_cigar2 calls with a doubled band (software/bwamem.c:1511-1518;
 * software/bwa.c:96-179: banded global alignment with traceback, ksw_global2,
 * software/ksw.c:501-584, then NM and MD), the squeeze of a leading or trailing
 * deletion and the clips (software/bwamem.c:1523-1547).  Host buffers in and out,
 * the resident .pac when pac == NULL.  regs[reg_off[r] .. reg_off[r+1]) are the
 * regions of read r in doubled coordinates, as smem_chain2aln returns them; rb,
 * re, qb, qe, truesc and w are read.  One smem_aln_t per region, in region
 * order; cigar_off / md_off need not ascend (the regions are classified and the
 * output space is claimed on the device).  bwa_fix_xref2 (software/bwamem.c:1500)
 * needs the contig table and stays with the caller: every region must already
 * lie within one contig, and pos is in concatenated coordinates (contig id and
 * offset are the caller's).  Limits: qe - qb <= 1024 and re - rb <= 2048;
 * a region outside them gets SMEM_ALN_REJECT and the call goes on.
 * SMEM_E_CAPACITY when cigar_cap words or md_cap bytes do not hold the output:
 * *n_cigar_words / *n_md_bytes then give the sizes a retry needs (on success,
 * the sizes used).  SMEM_E_ARG for query codes above 4, a region outside its
 * read and a missing resident .pac. */
int  smem_reg2aln(smem_gpu_t *gpu, int n_reads, const uint8_t *codes, const uint64_t *offs,
                  const smem_alnreg_t *regs, const uint64_t *reg_off,
                  const uint8_t *pac, int64_t l_pac, const smem_aln_opt_t *opt,
                  smem_aln_t *alns, uint32_t *cigar, uint64_t cigar_cap, uint64_t *n_cigar_words,
                  char *md, uint64_t md_cap, uint64_t *n_md_bytes, double *kernel_ms);

/* The contig table of the index, bns->anns[].offset / .len (software/bntseq.h), kept in HBM
 * for smem_batch_reg2aln: uploaded once per handle (again: replaced), freed at shutdown.
 * SMEM_E_ARG unless n_seqs > 0, offset[0] == 0, every len > 0, offset[i] + len[i] ==
 * offset[i + 1] and the last contig ends at l_pac.  Optional: without it (or when its l_pac
 * is not the resident .pac's) smem_batch_reg2aln gives rid -1 and marks nothing as bridging. */
int  smem_gpu_load_contigs(smem_gpu_t *gpu, int n_seqs, const int64_t *offset, const int32_t *len, int64_t l_pac);
/* Device-resident twin of smem_reg2aln: after smem_batch_reg_finalize, the alignment of every
 * record of the batch over the final regions, the reads and the resident .pac still in HBM;
 * no region, task or list crosses to the host.  idx == NULL: the records are
 * regs_out[sel_idx[..]] of smem_batch_reg_finalize, per read by sel_off.  Else the caller's
 * selection: idx[idx_off[r] .. idx_off[r + 1]) are read r's records as indices into the
 * batch's final regions, each within the read's [out_off[r], out_off[r + 1]) (duplicates
 * allowed); SMEM_E_ARG otherwise.  One smem_aln_t per record, as smem_reg2aln fills it, and
 * one rid: with a contig table, bns_pos2rid of the final pos (software/bwamem.c:1548; pos
 * itself stays in concatenated coordinates), and a region for which bwa_fix_xref2 would
 * change something gets SMEM_ALN_XREF and no alignment; without one, -1.  The CIGAR / MD pools
 * are the stage's own: sized from an estimate per record (SMEM_G2A_POOL=<words>:<bytes>
 * overrides it) and, when too small, grown to the sizes the kernels report before one more
 * pass -- the caller never sees SMEM_E_CAPACITY.  SMEM_E_ARG: smem_batch_reg_finalize has not
 * run on this batch, no resident .pac, bad scoring.  smem_batch_fetch_mask(b, SMEM_FETCH_ALN)
 * copies the results, smem_batch_aln2_results returns them (any pointer may be NULL; aln_off
 * [n_reads + 1] is sel_off or idx_off).  A later smem_batch_chain2aln or
 * smem_batch_reg_finalize on the batch ends them. */
int  smem_batch_reg2aln(smem_batch_t *b, const smem_aln_opt_t *opt, const uint64_t *idx, const uint64_t *idx_off);
int  smem_batch_aln2_results(const smem_batch_t *b, const smem_aln_t **alns, const int32_t **rid,
                             const uint64_t **aln_off, const uint32_t **cigar, uint64_t *n_cigar_words,
                             const char **md, uint64_t *n_md_bytes, uint64_t *n_alns);

/* ------------------------------------------- raw regions -> final regions */
/* the mem_opt_t fields the stage reads (software/bwamem.h:33-58) */
typedef struct {
	int a, b;                          /* 1, 4 */
	int o_del, e_del, o_ins, e_ins;    /* 6, 1, 6, 1 */
	int min_seed_len;                  /* 19 */
	int T;                             /* 30: minimum score to output */
	float mask_level;                  /* 0.50 */
	float mask_level_redun;            /* 0.95 */
	float mapQ_coef_len;               /* 50 */
	int mapQ_coef_fac;                 /* (int)log(50) = 3: an int in the reference (software/bwamem.h:56) */
	int flag;                          /* SMEM_FIN_F_* */
} smem_fin_opt_t;
#define SMEM_FIN_F_NO_EXACT 1          /* MEM_F_NO_EXACT: mem_test_and_remove_exact runs */
#define SMEM_FIN_F_ALL      2          /* MEM_F_ALL: secondary regions get records */
#define SMEM_FIN_F_NO_MULTI 4          /* MEM_F_NO_MULTI: 0x10000 instead of 0x800 */
void smem_fin_opt_default(smem_fin_opt_t *opt);
/* what mem_reg2sam_se / mem_reg2aln decide about one final region before they align it
 * (software/bwamem.c:1370-1379, 1498-1499, 1550): flag -1: the region gets no record; else the
 * bits 0x100 (secondary), 0x800 or 0x10000 (supplementary) -- 0x10 is the strand of rb, the
 * caller's; mapq after the cap at the read's first record, or -1: an argument of
 * mem_approx_mapq_se lies outside the stage's tables (max(qe - qb, re - rb), seedcov or sub_n
 * >= SMEM_FIN_TAB_LEN, seedcov < 1 where its log is needed, a region of length 0) and the
 * caller computes it -- the cap applies to -1 as to any number, so the records behind a first
 * record of -1 are -1 too; xs = max(sub, csub), -1 for a secondary region */
typedef struct { int32_t mapq, flag, xs; } smem_fin_sel_t;
#define SMEM_FIN_MAX_REGS 1024         /* raw regions of one read */
#define SMEM_FIN_TAB_LEN  4096
#define SMEM_FIN_REJECT   1
/* mem_sort_and_dedup (software/bwamem.c:705-746), mem_test_and_remove_exact (:748-753, with
 * SMEM_FIN_F_NO_EXACT), mem_mark_primary_se (:755-785) and the selection, MAPQ and flags at
 * the head of mem_reg2sam_se / mem_reg2aln, of every read on the GPU.  Host buffers in and
 * out.  regs[reg_off[r] .. reg_off[r+1]) are the raw regions of read r in the order
 * mem_chain2aln appended them (smem_chain2aln's output as it is), read_len[r] its length,
 * ids[r] the id its hashes start from (NULL: id0 + r; single-end n_processed + r, paired-end
 * id << 1 | end, software/bwamem.c:1604, software/bwamem_pair.c:264-265).
 * regs_out (room for reg_off[n_reads] regions) / out_off[n_reads + 1]: each read's final list
 * in mem_mark_primary_se's order with sub, sub_n (added to the incoming value, as the
 * reference does), secondary (an index within the read's list, -1: primary) and hash set;
 * sel: one per output region; sel_idx (room for reg_off[n_reads]) / sel_off[n_reads + 1]:
 * the regions that get a record, per read in print order, as indices into regs_out -- a read
 * with none gets the caller's unmapped record.  regs_out[sel_idx[..]] is smem_reg2aln's input.
 * status[r] (may be NULL): 0, or SMEM_FIN_REJECT for a read of more than SMEM_FIN_MAX_REGS
 * raw regions: it gets an empty list, the call goes on and the caller does that read on the
 * CPU.  SMEM_E_ARG: reg_off not ascending, a region with qe < qb, a negative read length. */
int  smem_reg_finalize(smem_gpu_t *gpu, int n_reads, const int *read_len, const smem_alnreg_t *regs,
                       const uint64_t *reg_off, const int64_t *ids, int64_t id0, const smem_fin_opt_t *opt,
                       smem_alnreg_t *regs_out, uint64_t *out_off, smem_fin_sel_t *sel, uint64_t *sel_idx,
                       uint64_t *sel_off, int32_t *status, double *kernel_ms);
/* Device-resident twin: after smem_batch_chain2aln, over the regions still in HBM (no host
 * round trip).  smem_batch_fetch_mask(b, SMEM_FETCH_FIN) copies the results, smem_batch_fin_results
 * returns them (any pointer may be NULL); SMEM_FETCH_REGS keeps returning the raw regions.  The
 * stage's buffers exist only in a batch that called it; smem_batch_stats' fin_ms is its kernel time. */
int  smem_batch_reg_finalize(smem_batch_t *b, const int64_t *ids, int64_t id0, const smem_fin_opt_t *opt);
int  smem_batch_fin_results(const smem_batch_t *b, const smem_alnreg_t **regs_out, const uint64_t **out_off,
                            const smem_fin_sel_t **sel, const uint64_t **sel_idx, const uint64_t **sel_off,
                            const int32_t **status, uint64_t *n_out, uint64_t *n_sel);

/* ------------------------------------------------------------ mate rescue */
/* The rescue loop of mem_sam_pe (software/bwamem_pair.c:252-263): for the good hits of either
 * end -- score >= the end's first region's score - pen_unpaired, at most max_matesw of them,
 * taken from the lists as they come in -- mem_matesw (:109-175) of the other end's read: a
 * ksw_align2 of the mate against the window the insert-size bounds give, in every orientation
 * that has not failed and that no region of the mate's current list already fills, the hit
 * inserted before the first lower score, then mem_sort_and_dedup.  End 0's anchors change end 1's
 * list; end 1's anchors then change end 0's.
 * mem_pestat_t (software/bwamem.h:78-82); the stage reads low, high and failed, which
 * smem_pestat computes. */
typedef struct {
	int32_t low, high, failed, pad;
	double avg, std;
} smem_pestat_t;
typedef struct {
	smem_ksw_opt_t sc;        /* matrix and gap penalties */
	int32_t a, min_seed_len;
	int32_t pen_unpaired;     /* 17 */
	int32_t max_matesw;       /* 100 */
	float mask_level_redun;   /* 0.95 */
	int32_t pad;
} smem_matesw_opt_t;
void smem_matesw_opt_default(smem_matesw_opt_t *opt);
#define SMEM_MSW_HOST 1
/* Host buffers in and out.  Reads 2p and 2p + 1 are pair p: codes (0..4) / offs[2 n_pairs + 1];
 * regs / reg_off[2 n_pairs + 1] are each read's regions as mem_align1_core leaves them (after
 * mem_sort_and_dedup), 0 <= qb < qe <= the read's length; pac NULL: the resident .pac of this
 * l_pac.  regs_out (room for regs_cap regions) / reg_off_out[2 n_pairs + 1] get both ends' lists
 * after the loop, n_sw[p] the n mem_sam_pe accumulates from mem_matesw's return values,
 * status[p] 0 or SMEM_MSW_HOST, *n_regs_out the regions written.  SMEM_MSW_HOST: the pair is
 * left to the caller's CPU path, its lists copied through and n_sw 0 -- a mate of 0 or more than
 * 256 bp, a list of more than SMEM_FIN_MAX_REGS regions (coming in, or after an insertion), or an
 * SW window longer than SMEM_KSWA_MAX_TLEN.  SMEM_E_CAPACITY when regs_cap is too small:
 * *n_regs_out is the size to come back with.  SMEM_E_ARG: offsets that do not ascend, a code
 * above 4, a region outside its read, no .pac, gap penalties with e < 1 or o < 0, a < 1. */
int  smem_matesw(smem_gpu_t *gpu, int n_pairs, const uint8_t *codes, const uint64_t *offs, const smem_alnreg_t *regs,
                 const uint64_t *reg_off, const smem_pestat_t pes[4], const uint8_t *pac, int64_t l_pac,
                 const smem_matesw_opt_t *opt, smem_alnreg_t *regs_out, uint64_t regs_cap, uint64_t *reg_off_out,
                 int32_t *n_sw, int32_t *status, uint64_t *n_regs_out, double *kernel_ms);

/* ------------------------------------------- insert-size statistics and pairing */
/* the mem_opt_t fields mem_pestat reads */
typedef struct {
	int32_t a, min_seed_len;  /* 1, 19 */
	int32_t max_ins;          /* 10000; 1 .. SMEM_PESTAT_MAX_INS */
	float mask_level;         /* 0.50 */
	int32_t pad[2];
} smem_pestat_opt_t;
void smem_pestat_opt_default(smem_pestat_opt_t *opt);
#define SMEM_PESTAT_MAX_INS 65535
/* mem_pestat (software/bwamem_pair.c:46-107).  Host buffers in and out.  Reads 2p and 2p + 1 are
 * pair p; regs / reg_off[2 n_pairs + 1] are each read's list as mem_align1_core leaves it (after
 * mem_sort_and_dedup, before mem_mark_primary_se), smem_matesw's input.  On the device, a lane per
 * pair (:52-63): a pair with an empty end is skipped, cal_sub (:32-44) of both ends -- a sequential
 * scan over a list of any length that stops at the first significant overlap, the float product
 * min_l * mask_level compared as the reference compares it --, the two tests against MIN_RATIO *
 * score in double, mem_infer_dir of the two first regions, and where 0 < is <= max_ins one count
 * into a histogram hist[dir][is].  The histogram, 4 * (max_ins + 1) counts, is what crosses to the
 * host, which runs :64-106 over it in ascending order and in the reference's order of operations:
 * the sum of squares takes one addition per pair, value by value, as the loop over the sorted
 * array does.  pes[d]: low, high, failed, avg and std as mem_pestat leaves them (d = FF, FR, RF,
 * RR), a failed orientation all zeros apart from failed; n_cand[d]: the "# candidate unique
 * pairs".  n_pairs == 0 is valid and gives four failed orientations.  SMEM_E_ARG: max_ins < 1 or
 * > SMEM_PESTAT_MAX_INS, a < 1, min_seed_len < 0, a mask_level that is NaN, reg_off that does not
 * ascend, a missing buffer. */
int  smem_pestat(smem_gpu_t *gpu, int n_pairs, const smem_alnreg_t *regs, const uint64_t *reg_off,
                 int64_t l_pac, const smem_pestat_opt_t *opt, smem_pestat_t pes[4],
                 uint64_t n_cand[4], double *kernel_ms);

/* the mem_opt_t fields mem_pair, the decision block of mem_sam_pe and mem_approx_mapq_se read */
typedef struct {
	int32_t a, b;                      /* 1, 4 */
	int32_t o_del, e_del, o_ins, e_ins;/* 6, 1, 6, 1 */
	int32_t pen_unpaired;              /* 17 */
	int32_t T;                         /* 30 */
	int32_t min_seed_len;              /* 19 */
	float mapQ_coef_len;               /* 50 */
	int32_t mapQ_coef_fac;             /* 3 */
	int32_t flags;                     /* SMEM_PAIR_F_* */
} smem_pair_opt_t;
#define SMEM_PAIR_F_NOPAIRING 1        /* MEM_F_NOPAIRING */
void smem_pair_opt_default(smem_pair_opt_t *opt);
#define SMEM_PAIR_TAB_LEN 65536        /* the longest range high - low + 1 of a live orientation */
#define SMEM_PAIR_HOST    1
/* what mem_sam_pe decides about one pair between mate rescue and mem_reg2aln (:266-304, :321-326) */
typedef struct {
	int32_t status;      /* 0, or SMEM_PAIR_HOST: the pair is the caller's and every other field is 0 -- an
	                        end of more than SMEM_FIN_MAX_REGS regions; n_sub >= SMEM_FIN_TAB_LEN where line
	                        282 needs its logarithm; an argument of mem_approx_mapq_se outside the finalize
	                        stage's tables (smem_fin_sel_t's cases) for a region lines 292, 302-303 score */
	int32_t branch;      /* 0: no pairing (MEM_F_NOPAIRING, an empty end, mem_pair returned 0, or is_multi of
	                        either end, :271-276); 1: the paired alignment is preferred (o > score_un, :286);
	                        2: the unpaired one (:300) */
	int32_t z[2];        /* the regions to print, as indices into each end's list: mem_pair's in branch 1,
	                        0, 0 otherwise */
	int32_t mapq[2];     /* q_se after :294-299 (branch 1) or :302-303 (branch 2); -1 in branch 0, where the
	                        single-end selection has them */
	int32_t proper;      /* extra_flag & 2.  Branch 0: the test of :324-325 on the two first regions, made
	                        where both ends have one with score >= T and 0 elsewhere; h[0].rid == h[1].rid
	                        >= 0 of :321 needs the alignments' contigs and stays the caller's AND */
	int32_t o, subo, n_sub;   /* as mem_pair returns them (subo before :280's max); 0 where it did not run */
	int32_t sub[2], promoted[2];   /* branch 1: the chosen region's sub after :291 and whether its secondary
	                        became -2; the lists are not written back */
} smem_pair_sel_t;
/* mem_pair (:177-236) and the decision block around it for every pair, on the GPU.  Host buffers
 * in and out.  regs / reg_off[2 n_pairs + 1] are each read's list after mem_mark_primary_se(...,
 * id << 1 | end), the order smem_reg_finalize writes, with secondary (an index into the read's
 * list, or < 0), sub, sub_n and csub set; ids[p] the pair's id (NULL: id0 + p), (n_processed >> 1)
 * + i of software/bwamem.c:1609 -- an int in mem_pair, so its low 32 bits count; pes: smem_pestat's
 * result.  Before the launch the host fills, for every orientation that has not failed, pen[d][dist
 * - low] = .721 * log(2. * erfc(fabs((dist - avg) / std) * M_SQRT1_2)) * a for dist in [low, high]
 * with its own libm; the device adds (double)(s_i + s_k), the entry and .499, two IEEE additions,
 * and truncates -- a sum that is not finite or is negative gives q = 0.  Keys (:186-187) are sorted
 * as 128-bit pairs; the walk-back scan (:194-220) is the reference's; the array u is not built: the
 * largest (q << 32 | hash, k << 32 | i), the second's q and n_sub are kept.  A pair of up to 16
 * regions in both lists is done by one lane, a longer one by one wave with the keys in LDS.
 * sel: one per pair.  SMEM_E_ARG (before any device work): a range high - low + 1 above
 * SMEM_PAIR_TAB_LEN in an orientation that has not failed, reg_off that does not ascend, a
 * secondary at or past its list's length, a negative score, a < 1, b < 0, unknown flags, a
 * mapQ_coef_len that is NaN, a missing buffer. */
int  smem_pair(smem_gpu_t *gpu, int n_pairs, const smem_alnreg_t *regs, const uint64_t *reg_off,
               const int64_t *ids, int64_t id0, int64_t l_pac, const smem_pestat_t pes[4],
               const smem_pair_opt_t *opt, smem_pair_sel_t *sel, double *kernel_ms);

/* ------------------------------------------- alignments -> SAM text */
/* The text mem_reg2sam_se(opt, bns, pac, s, a, 0, 0) leaves in s->sam (software/bwamem.c:1359-1393,
 * through mem_aln2sam, :1214-1327) for every read, on the GPU: single end, no mate, no XA; one
 * line per record of the read's list in list order (SA:Z from the read's own records, hard clips
 * and a trimmed SEQ / QUAL on every record after the first), or the unmapped line (flag 4,
 * AS:i:0, XS:i:0) for a read without a record.  No @ header lines. */
#define SMEM_SAM_HOST 1
/* status of a read the stage leaves to the caller, the reference's reject -> CPU convention: one
 * of its records has a status other than 0 (SMEM_ALN_XREF, _REJECT, _NOCIGAR, _UNMAPPED) or
 * mapq -1, its finalize status is SMEM_FIN_REJECT, or its length is 0.  The read gets zero bytes
 * (all of its lines: the SA:Z of its other records would need the missing alignment). */
typedef struct {
	const char *rg_id;       /* bwa_rg_id: NULL or "": no RG:Z tag (at most 1023 bytes) */
} smem_sam_opt_t;
/* what mem_reg2sam_se decides about a record beside its alignment: finalize's capped mapq and
 * flag (0x100, 0x800, 0x10000; 0x10 comes from the alignment's strand), the final region's
 * score (AS) and xs (XS; -1: none) */
typedef struct { int32_t mapq, flag, score, xs; } smem_sam_rec_t;
/* bns->anns[].name beside the table of smem_gpu_load_contigs: name i is names[name_off[i] ..
 * name_off[i + 1]).  SMEM_E_ARG unless a contig table of the same n_seqs is loaded.  Loading
 * again replaces the names; loading another contig table drops them; freed at shutdown. */
int  smem_gpu_load_contig_names(smem_gpu_t *gpu, int n_seqs, const char *names, const uint64_t *name_off);
/* The text of the batch's reads (after smem_batch_set_reads*): read r's name is names[name_off[r]
 * .. name_off[r + 1]), at most 255 bytes (more: SMEM_E_ARG); qual (NULL: the stage prints '*')
 * holds the reads' qualities one after the other in batch order, as the codes were given;
 * comments / comment_off (NULL: none; an empty comment: none) as the names.  Copied through
 * pinned batch memory.  A later smem_batch_set_reads* ends them. */
int  smem_batch_set_read_text(smem_batch_t *b, const char *names, const uint64_t *name_off, const char *qual,
                              const char *comments, const uint64_t *comment_off);
/* After smem_batch_reg2aln (idx == NULL: only the finalize selection has MAPQ and flags per record)
 * with a contig table, contig names and read text: every read's lines, in HBM.  Two passes with
 * one 8-byte total read in between: the lengths (per record, per read, the offset scan), then
 * the text; the text buffer grows to the total when it is too small, so the caller never sees
 * SMEM_E_CAPACITY.  SMEM_E_ARG when one of the above is missing.  smem_batch_fetch_mask(b,
 * SMEM_FETCH_SAM) copies the results; smem_batch_sam_results returns them (any pointer may be
 * NULL): text[text_off[r] .. text_off[r + 1]) are read r's lines, reads in batch order (a batch
 * whose reads all have status 0 can be written to a file as it is), status[r] is 0 or
 * SMEM_SAM_HOST.  A later smem_batch_chain2aln, _reg_finalize or _reg2aln ends the results. */
int  smem_batch_sam(smem_batch_t *b, const smem_sam_opt_t *opt);
int  smem_batch_sam_results(const smem_batch_t *b, const char **text, const uint64_t **text_off,
                            const int32_t **status, uint64_t *n_bytes);
/* The stage's statistics of the batch's last smem_batch_sam (zero before it).  They have a
 * struct of their own: smem_batch_stats_t keeps its size and every member its place. */
typedef struct {
	double sam_ms;           /* the length pass (with its scan) + the write pass, HIP events */
	uint64_t n_sam_bytes;    /* bytes of text written */
	uint64_t n_sam_host;     /* reads left to the caller (SMEM_SAM_HOST) */
	double sam_write_ms;     /* the write pass alone (tools/samtext_time.py: its bytes per second) */
} smem_sam_stats_t;
int  smem_batch_sam_stats(const smem_batch_t *b, smem_sam_stats_t *st);
/* The same over host buffers.  Reads: codes (0..4) / offs[n_reads + 1], names / name_off, qual
 * (by offs; NULL: '*'), comments / comment_off (NULL: none).  Records: read r's are
 * [aln_off[r], aln_off[r + 1]) (aln_off[0] == 0), each an smem_aln_t with its CIGAR / MD in the
 * pools (smem_reg2aln's or smem_batch_aln2_results' layout; pos in concatenated coordinates), its
 * contig rid and an smem_sam_rec_t; fin_status (NULL: all 0) per read.  Contigs: offset[n_seqs]
 * and names by ctg_name_off[n_seqs + 1].  text (text_cap bytes), text_off[n_reads + 1] and
 * status[n_reads] are filled; *n_bytes gets the text's size.  SMEM_E_CAPACITY when text_cap is
 * too small: *n_bytes (and text_off, status) then give what a retry needs.  kernel_ms (may be
 * NULL): both passes.  Arguments are checked on the host before any device is touched:
 * SMEM_E_ARG for gpu == NULL, offsets that do not ascend, a name over 255 bytes, a code above 4,
 * and a record of status 0 whose rid, CIGAR or MD lies outside what was passed. */
int  smem_sam_text(smem_gpu_t *gpu, int n_reads, const uint8_t *codes, const uint64_t *offs, const char *names,
                   const uint64_t *name_off, const char *qual, const char *comments, const uint64_t *comment_off,
                   const uint64_t *aln_off, const smem_aln_t *alns, const int32_t *rid, const smem_sam_rec_t *recs,
                   const int32_t *fin_status, const uint32_t *cigar, uint64_t n_cigar_words, const char *md,
                   uint64_t n_md_bytes, int n_seqs, const int64_t *ctg_offset, const char *ctg_names,
                   const uint64_t *ctg_name_off, const smem_sam_opt_t *opt, char *text, uint64_t text_cap,
                   uint64_t *text_off, int32_t *status, uint64_t *n_bytes, double *kernel_ms);

/* The paired-end text: the tail of mem_sam_pe (software/bwamem_pair.c:305-331) through mem_aln2sam
 * with a mate (software/bwamem.c:1219-1260), smem_sam_text's arguments and conventions with n_pairs
 * and sel, smem_pair's output unchanged.  Reads 2p and 2p + 1 are pair p (n_reads == 2 n_pairs).
 * Records, per read, in smem_sam_text's layout: in branch 0 the finalize selection's list (it may
 * be empty: mem_reg2sam_se prints the unmapped record); in branch 1 and 2 exactly one record, the
 * alignment of region z[e] with xs = max(sub, csub) (sub after line 291) and flag 0 -- its
 * recs[].mapq is ignored and sel[p].mapq[e] printed.  From sel[p] the stage takes status, branch,
 * mapq and proper; it derives the rest: the mate of every line of read r is record 0 of read r ^ 1,
 * or unmapped when that read has no record; 0x1, 0x40 / 0x80, 0x8, 0x20; 0x2 from proper, in branch
 * 0 only where both reads have a record 0 on one contig (:321); an unmapped read whose mate is
 * mapped prints the mate's RNAME and POS, MAPQ 0 and CIGAR *, and with a reverse mate 0x10 and its
 * SEQ / QUAL reverse-complemented / reversed; a mapped read whose mate is not prints =, its own
 * POS and 0 with 0x20 from its own strand; RNEXT is = or the mate's contig, PNEXT the mate's POS,
 * TLEN -(p0 - p1 + sign(p0 - p1)) over the 5' ends (a reverse alignment adds the M and D lengths
 * of its CIGAR less one), 0 across contigs or where either side has no CIGAR, per line against
 * the same mate.  Everything from SEQ on is smem_sam_text's.
 * status: a pair is the caller's (SMEM_SAM_HOST for both reads, zero bytes for both) when
 * sel[p].status != 0 or either read meets one of smem_sam_text's conditions (in branch 1 and 2 a
 * sel[p].mapq[e] of -1 stands for the record's).  SMEM_E_ARG, before any device work:
 * n_reads != 2 n_pairs, a pair whose reads' names differ (err_fatal in the reference), a branch
 * outside 0..2, a read of a pair in branch 1 or 2 without exactly one record, and smem_sam_text's
 * cases.  SMEM_E_CAPACITY and its retry as smem_sam_text.  n_pairs == 0 is valid. */
int  smem_sam_text_pe(smem_gpu_t *gpu, int n_pairs, const smem_pair_sel_t *sel, int n_reads, const uint8_t *codes,
                      const uint64_t *offs, const char *names, const uint64_t *name_off, const char *qual,
                      const char *comments, const uint64_t *comment_off, const uint64_t *aln_off,
                      const smem_aln_t *alns, const int32_t *rid, const smem_sam_rec_t *recs,
                      const int32_t *fin_status, const uint32_t *cigar, uint64_t n_cigar_words, const char *md,
                      uint64_t n_md_bytes, int n_seqs, const int64_t *ctg_offset, const char *ctg_names,
                      const uint64_t *ctg_name_off, const smem_sam_opt_t *opt, char *text, uint64_t text_cap,
                      uint64_t *text_off, int32_t *status, uint64_t *n_bytes, double *kernel_ms);

/* ---------------------------------------------------------- telemetry */
typedef struct {
	double kernel_ms;        /* seeding kernel(s), HIP events on the batch stream */
	double compact_ms;       /* result compaction kernels */
	uint64_t n_intv;         /* intervals produced */
	uint64_t n_calls;        /* smem_next2 lists produced */
	uint32_t n_overflow;     /* reads re-run with a larger output capacity */
	int grid, block;         /* launch shape of the seeding kernel */
	double sa_ms;            /* smem_batch_sa kernels */
	uint64_t n_occ;          /* seed occurrences resolved by smem_batch_sa */
	double chain_ms;         /* smem_batch_chain kernels */
	uint64_t n_chains;       /* chains kept by smem_batch_chain */
	double aln_ms;           /* smem_batch_chain2aln kernels */
	uint64_t n_regs;         /* regions made by smem_batch_chain2aln */
	uint64_t t_start, t_end; /* the seeding launches' first wave start and last wave end, chip-wide
	                          * 100 MHz clock (s_memrealtime): comparable across batches and streams */
	double fin_ms;           /* smem_batch_reg_finalize kernels; fin_lane_ms / fin_wave_ms: its two tiers */
	double fin_lane_ms, fin_wave_ms;
	uint64_t n_fin, n_fin_sel; /* final regions, regions with a record */
	double g2a_ms;           /* smem_batch_reg2aln: prep + DP kernels (every pass); g2a_prep_ms: the prep kernel */
	double g2a_prep_ms;
	uint64_t n_g2a;          /* records; n_g2a_deferred: regions redone by the scratch tier; n_g2a_xref: SMEM_ALN_XREF */
	uint64_t n_g2a_deferred, n_g2a_xref;
	uint64_t n_g2a_passes;   /* 1, or 2 when the CIGAR / MD pools had to grow */
} smem_batch_stats_t;
int  smem_batch_stats(const smem_batch_t *b, smem_batch_stats_t *st);

/* tuning knobs (0 = default) — lanes per CU of the persistent seeding grid
 * (default: the kernel's own -- 960 for the 4-block seed_wp_kernel variants,
 * 768 otherwise) */
int  smem_gpu_set_lanes_per_cu(smem_gpu_t *gpu, int lanes_per_cu);
/* per-read output capacity (intervals) of batches created afterwards;
 * reads needing more go through the overflow pass (0 = len/2 + 32) */
int  smem_gpu_set_intv_cap(smem_gpu_t *gpu, int cap_per_read);
/* seeding-kernel variant, all bit-exact, kept for A/B measurement (the
 * product build has 0 = 49 (the default, seed_wp_kernel: see
 * smem_gpu_get_kernel_variant below for 40-51), 2 = 20 = 26, 9, 23, 24, 25, 27
 * and 28; the others need a library built with `make AB=1`, else SMEM_E_ARG):
 * 2 (the default of rounds 1-4) Occ64 buckets (32 B per 64 symbols: three counts and
 * the symbols as two 64-bit bit planes, re-laid on the device at init), per-lane fetch into two register slots with bucket reuse,
 * the first 11 entries of every list in LDS (the forward list as a ring of its
 * last 11 pushes); 11 the same with LDS-DMA slots and 7 list entries; 12 that
 * with 12 LDS entries at 2 blocks per CU; 13 the round-1 default (LDS-DMA
 * slots, 7 entries, forward list in the arena); 16-18 variant 11 with two
 * backward extends per lane per iteration (16; 17/18 at 2 blocks per CU with
 * 12/13 entries); 19 the default with two extends when both hit the slots;
 * 20 = 2; 21 register slots, 7 entries, 4 blocks per CU; 3 reference-layout buckets,
 * cooperative fetch, lists in global memory; 4 reference layout, per-lane
 * fetch; 5 as 2 with 12 list entries in LDS (2 blocks per CU); 6 as 2 with
 * lists in global memory; 9 the default with per-wave cycle stamps; 24 the next read claimed in the
 * uniform section (25 stamped); 27 wave priority in the extend arithmetic instead; 28 no wave priority
 * (smem_batch_debug); 10 the default on the Occ192 layout (64-B lines of
 * 192 symbols, built on first use: exact, 7 % slower at human size); 22
 * register slots on Occ192; 23 the default reading the bi-interval of every
 * extend result of at most k bases from the k-mer table (needs
 * smem_gpu_set_kmer_table) */
int  smem_gpu_set_kernel_variant(smem_gpu_t *gpu, int variant);
/* the seeding kernel variant the handle is set to (0 given to the setter = the
 * default, 49: seed_wp_kernel -- the backward steps' entries extended by the
 * whole wave and pruned by ballot / prefix rank (software/bwt.c:812-826), 24
 * reads owned per wave, 18 list entries per read in LDS, 4 blocks per CU.
 * A handle left on the default runs that shape's instantiation 68, which
 * keeps the entries whose strings the handle's k-mer table answers virtual
 * (smem_gpu_kmer_facts), while it holds a table of depth >= 2;
 * smem_gpu_seed_kernel returns the instantiation the next launch runs.
 * 68 does the extend's rank arithmetic in 32 bits, which is exact while every
 * base occurs fewer than 2^32 times in the BWT (smem_occ_narrow_ok below); a
 * handle on another index, or made with SMEM_GPU_OCC_WIDE=1 in the
 * environment, runs 71 in its place: the same kernel with 64-bit counts.
 * 49 set by number (or SMEM_GPU_SEED_VARIANT=49) is the plain kernel, in every
 * build, for A/B; 68 by number runs it whatever the table (none: 49's path).
 * Mind the collision: the number this getter reports for a default handle (49)
 * is also the plain kernel's, and bench.py / tools/traffic.py key the recorded
 * counters (profiles/traffic*.json) by it.  The committed records hold kernel
 * 68's counters at its default depth under "variant": 49, so the roofline and
 * counter fields bench.py prints for a `--variant 49` run, or for a run with
 * another SMEM_GPU_KMER_K, are those records', not that run's.
 * A/B (make AB=1): 69, 70 = 68 with 32 reads / 12 entries, 28 / 14; 40 32 reads / 20 entries / 3 blocks; 41 32 / 16; 42 24 / 24; 43 = 40
 * without wave priority; 44 24 / 16 / 4 blocks; 45 32 / 12; 46 28 / 14; 47, 48
 * two entries per worker lane; 50 20 / 22; 51 = 44 without wave priority; 2:
 * the lane-per-read seed_kernel of rounds 1-4).  SMEM_GPU_SEED_VARIANT in the
 * environment sets the default of every handle opened afterwards. */
int  smem_gpu_get_kernel_variant(const smem_gpu_t *gpu);
int  smem_gpu_seed_kernel(smem_gpu_t *gpu);
/* build (k = 1..15) or free (k = 0) the device table of the bi-intervals of
 * every string of 1..k bases, built on the device from the resident index:
 * 16 B x (4^(k+1) - 4) / 3 (k = 12: 358 MB, 14: 5.7 GB); a table of a string
 * is the interval bwt_extend reaches for it on any path (software/bwt.c:416-429) */
int  smem_gpu_set_kmer_table(smem_gpu_t *gpu, int k);
/* A handle builds this table for itself when the index is loaded (k = 12, or
 * SMEM_GPU_KMER_K from the environment; no deeper than 4^k <= the index's
 * length; at 12 levels with a leaf level behind them, below; k = 0 or a
 * failed allocation: no table, the plain path), and
 * smem_gpu_set_kmer_table replaces or removes it.  The table's facts: *k its
 * depth (0: none), minsz[L] the smallest interval size among the strings of L
 * bases (0: one is absent; L = 1..k, n_minsz words written), *depth the
 * largest level D < k such that every string of D + 1 bases occurs.  A
 * bwt_smem1 call skips the extends of strings of fewer than
 * smem_kmer_leaf_probe_depth(...) bases (below: D, or k where the unstored
 * level k + 1 is complete too, or k + 1 where a leaf vouches for itself), min_intv taken as
 * start_width for a read's first calls and as split_width + 1 (the most a
 * re-seeding call can ask for) for its re-seeding calls. */
int  smem_gpu_kmer_facts(smem_gpu_t *gpu, int *k, int *depth, uint64_t *minsz, int n_minsz);
/* the two choices above as host functions of a table's per-level minimum
 * sizes mn[1..k] (mn[0] unused) */
int  smem_kmer_depth(const uint64_t *mn, int k);
int  smem_kmer_call_depth(const uint64_t *mn, int depth, int64_t min_intv);
/* The depth a launch really probes at.  *depth above stops at k - 1 because
 * level D + 1 has to be seen complete, and smem_gpu_kmer_facts only reports
 * the stored levels.  The build also reduces level k + 1, computed from level
 * k and the index and never stored, to its smallest size (min_next; 0 or
 * UINT64_MAX: a string of k + 1 bases is absent, or the level was not
 * reduced, which is the case for k = 15).  smem_kmer_probe_depth is the
 * largest level L <= k with levels 1 .. L + 1 all complete and
 * mn[L] >= min_intv (min_intv < 1 taken as 1): k itself where all k levels
 * and the unstored one are complete, and
 * smem_kmer_call_depth(mn, smem_kmer_depth(mn, k), min_intv) otherwise.  So
 * the reported D and the kernel's depth may differ by one: D counts the
 * levels the table stores, the kernel may also rely on the one reduced beside
 * them.  smem_gpu_kmer_probe_depth returns that depth for the handle's table
 * (0: no table) and writes the unstored level's minimum to *min_next (may be
 * NULL); a batch run passes it for min_intv = start_width and for
 * split_width + 1. */
int  smem_kmer_probe_depth(const uint64_t *mn, int k, uint64_t min_next, int64_t min_intv);
int  smem_gpu_kmer_probe_depth(smem_gpu_t *gpu, int64_t min_intv, uint64_t *min_next);
/* The leaf.  Behind the k levels it reports a table may store one more, level
 * k + 1, in the same allocation (16 B x 4^(k+1) more; at k = 12: 1.07 GB, the
 * table 1.43 GB).  smem_gpu_init builds it when the table has the default's 12
 * levels and 4^13 <= the index's length (SMEM_GPU_KMER_LEAF=0: never; if the
 * larger allocation fails, the 12 levels alone are tried before the plain
 * kernel); smem_gpu_set_kmer_table_leaf builds k levels (1..13) and a leaf on
 * any index; smem_gpu_set_kmer_table builds exactly k levels and no leaf.
 * smem_gpu_kmer_facts reports the same k, D and minsz with or without a leaf,
 * and *min_next above is then the leaf's own minimum.  While the leaf is built
 * the four one-base extensions of each of its strings are formed once: their
 * minimum is level k + 2's (next_min; 0: a string is absent), and *strict
 * tells that no present string of k + 1 bases has an extension of its own
 * size.  smem_kmer_leaf_probe_depth is the depth a launch takes: k + 1 when
 * levels 1 .. k + 1 are complete, min_next >= min_intv, and the leaf is strict
 * or level k + 2 is complete (which implies it); smem_kmer_probe_depth's
 * answer otherwise and whenever leaf == 0.  It reads mn[1 .. k] only and
 * answers at most 15.  smem_gpu_kmer_probe_depth returns it for the handle's
 * table, so it may be k + 1.  smem_gpu_kmer_leaf_facts: *level k + 1 (0: the
 * handle's table has no leaf, and the other three are 0), *leaf_min its
 * smallest size, *strict, *next_min (any may be NULL). */
int  smem_gpu_set_kmer_table_leaf(smem_gpu_t *gpu, int k);
int  smem_kmer_leaf_probe_depth(const uint64_t *mn, int k, uint64_t min_next, int leaf, int leaf_strict,
                                uint64_t leaf_next, int64_t min_intv);
int  smem_gpu_kmer_leaf_facts(smem_gpu_t *gpu, int *level, uint64_t *leaf_min, int *strict, uint64_t *next_min);
/* The Occ64 rank on the host (diagnostics; no device is touched): the code of
 * the kernels, compiled for the CPU, so that its arithmetic can be checked on
 * counts no small index reaches.  smem_occ_narrow_ok: 1 when every base
 * occurs fewer than 2^32 times (L2[c + 1] - L2[c] < 2^32, c = 0..3), the
 * condition under which the seeding kernel's 32-bit extend is exact.
 * smem_occ64_host: the Occ64 layout (2 * n_ref buckets of 8 words into out)
 * of n_ref reference buckets of 16 words, as the device builds it at load.
 * smem_extend_host: one bwt_extend for base c (0..3) of the interval (a, b, s)
 * from the two Occ64 buckets (8 words each; the same pointer when k and l
 * share one) of rows kk = k - (k >= primary) and ll, k = a - 1, l = k + s;
 * narrow != 0: the 32-bit form.  out: the child's a-side start, b-side start
 * and size. */
int  smem_occ_narrow_ok(const uint64_t L2[5]);
int  smem_occ64_host(const uint32_t *bwt, uint64_t n_ref, uint32_t *out);
int  smem_extend_host(const uint32_t *bucket_k, const uint32_t *bucket_l, uint64_t kk, uint64_t ll, uint64_t a,
                      uint64_t b, uint64_t s, int c, uint64_t primary, const uint64_t L2[5], int narrow,
                      uint64_t out[3]);
/* variant 9 (stamped diagnostic build): copy the per-wave cycle split
 * {advance, fetch, compute, iterations, active lanes, t0, t1, 0} of the last
 * run; returns the number of words copied or a negative code */
int  smem_batch_debug(const smem_batch_t *b, uint64_t *out, uint64_t n_words);
const char *smem_strerror(int code);
/* content hash (16 hex digits) of the sources this library was built from
 * (bwa-mem-harp2_amd/Makefile SRC_HASH): lets a caller prove that the .so it
 * loaded is the build of the sources beside it */
const char *smem_gpu_build_id(void);
/* hash of the seeding kernel's own sources and compile flags only
 * (csrc/smem_kernels.hip / .h, csrc/occ_rank.h): a counter profile of seed_kernel recorded on
 * another build of the runtime still describes this one when it matches */
const char *smem_gpu_kernel_id(void);

#ifdef __cplusplus
}
#endif
#endif
