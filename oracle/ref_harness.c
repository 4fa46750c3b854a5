/*
 * ref_harness.c — TEST INFRASTRUCTURE ONLY.  Drives the *unmodified* reference
 * C sources (compiled in place from /root/reference/software by
 * oracle/Makefile into oracle/_ref/) so that golden vectors and the
 * "reference" CPU baseline come from the reference itself.  Nothing in the
 * product links this file.
 *
 * Commands
 *   index <in.fa> <prefix>
 *       bwa_index(-a is) — software/bwtindex.c:187 (BWT by software/is.c:208,
 *       Occ interleave by software/bwtindex.c:128-150, .bwt dump software/bwt.c:841)
 *   smem  <in.bwt> <reads.smrd> <out.smgo> <k> <split_factor> <split_width> <start_width>
 *       For every read, the mem_chain() guard (software/bwamem.c:600) and the
 *       mem_insert_seed() loop (software/bwamem.c:453-460) calling the
 *       reference smem_next2() (software/bwamem.c:244); every returned list
 *       is written in SMGO format (include/smem_formats.h).
 *   bench <in.bwt> <reads.smrd> <n_threads> <max_reads> <k> <split_factor> <split_width> <start_width>
 *       Same loop, timed, pthreads over contiguous read chunks; prints one
 *       line: "reads=<n> seconds=<t> threads=<T> reads_per_s=<r>".
 *   sa    <in.bwt> <in.sa> <in.smgo> <out.smsa> <k> <max_occ>
 *       For every interval of the SMGO stream that mem_insert_seed() turns
 *       into seeds (software/bwamem.c:467), the reference bwt_sa()
 *       (software/bwt.c:104-114) of each occurrence x0 + j, j < x2
 *       (software/bwamem.c:469-474), written as SMSA (include/smem_formats.h).
 *   chain <in.bwt> <in.sa> <reads.smrd> <out.smch> <k> <r> <s> <start_width> <max_occ> <w>
 *         <max_chain_gap> <mask_level> <drop_ratio> <filter>
 *       For every read, the reference mem_chain() (software/bwamem.c:593) and,
 *       when filter != 0, mem_chain_flt() (software/bwamem.c:629) as
 *       mem_align1_core calls them (software/bwamem.c:1448-1449); chains
 *       written as SMCH (include/smem_formats.h).
 *   aln   <in.bwt> <in.sa> <in.pac> <reads.smrd> <out.smrg> <k> <r> <s> <start_width> <max_occ> <w>
 *         <max_chain_gap> <mask_level> <drop_ratio>
 *         [<a> <b> <o_del> <e_del> <o_ins> <e_ins> <zdrop> <pen_clip5> <pen_clip3>]
 *       mem_chain + mem_chain_flt as for chain (filter on), then per chain
 *       mem_chain2aln_short and, when it declines, mem_chain2aln
 *       (software/bwamem.c:1452-1460); every read's regions written as SMRG (and the
 *       wall time of the chain2aln loop alone on stderr: "chain2aln_seconds=..."):
 *       "SMRG0001", u64 n_reads, per read u32 n then n x {i64 rb, re;
 *       i32 qb, qe, score, truesc, sub, csub, sub_n, w, seedcov, secondary}.
 *       The nine optional scoring fields of mem_opt_t are taken literally (no
 *       -A scaling) and bwa_fill_scmat is called after them.
 *   kswa  <tasks.smat> <out.smar>
 *       the reference's own ksw_align2 (software/ksw.c:342) on every task
 *       (SMAT: as SMKT with per task {u64 q_off, t_off; i32 qlen, tlen, xtra, pad}),
 *       results as SMAR: "SMAR0001", u64 n, n x i32 {score, te, qe, score2, te2, tb, qb}.
 *   msw   <in.smmi> <out.smmo>
 *       the reference's own mem_matesw (software/bwamem_pair.c:109) on given lists, driven
 *       per pair as mem_sam_pe drives it (:252-263): each end's regions within
 *       pen_unpaired of its first are copied, the first max_matesw of them rescue the
 *       other end, end 0's first, and the returns are summed.  No limit on mate
 *       length, window or list length.
 *       SMMI: "SMMI0001", i64 l_pac, i32 pes[4] x {low, high, failed},
 *       i32 {a, b, o_del, e_del, o_ins, e_ins, min_seed_len, pen_unpaired, max_matesw, 0},
 *       f32 mask_level_redun, u64 {n_pairs, n_pac, n_codes, n_regs}, the .pac bytes,
 *       the reads' codes, u64 offs[2 n_pairs + 1], u64 reg_off[2 n_pairs + 1], n_regs x
 *       {i64 rb, re; i32 qb, qe, score, truesc, sub, csub, sub_n, w, seedcov, secondary; u64 hash}.
 *       SMMO: "SMMO0001", u64 n_pairs, u64 n_regs, i32 n[n_pairs] (the summed returns),
 *       u64 reg_off[2 n_pairs + 1], the lists afterwards as n_regs regions.
 *   mem   <prefix> <reads.fq> <n_threads> <batch_size> <pe> [<pg> [-k|-w|-A|-B|-O|-E|-L|-d <value>]...]
 *       The body of the reference's main_mem (software/fastmap.c:193-230) on the
 *       unmodified pipeline: bwa_print_sam_hdr, then bseq_read chunks through
 *       mem_process_seqs (software/bwamem.c:1614: kt_for_batch -> worker1_batched
 *       -> mem_align1_core_batched, then mem_sam_pe / mem_reg2sam_se), SAM on
 *       stdout.  The index is loaded as bwa_idx_load does (software/bwa.c:312-333)
 *       minus bwa_idx_load_bwt's FPGA upload (software/bwa.c:283-307), and the
 *       per-worker buffers main_mem allocates for the HARP path
 *       (software/fastmap.c:208-210; sw_handshake as the manager allocates it,
 *       :324) are allocated the same way.  With batch_size <= 2 every batch takes
 *       bwt_smem1_batched's CPU path (software/bwt.c:603, 686-717): this is
 *       `bwa mem -t N -b 1` of the reference, the golden SAM for the GPU build.
 *       The options after <pg> are read as main_mem reads them
 *       (software/fastmap.c:54-94), -A scaling what was not given (:159-171).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <pthread.h>
#include <sys/time.h>

#include <zlib.h>
#include "bwt.h"
#include "bwamem.h"
#include "bwa.h"
#include "bntseq.h"
#include "kseq.h"
#include "utils.h"
#include "ksw.h"
#include "smem_formats.h"
KSEQ_DECLARE(gzFile)

/* defined in software/bwamem.c:244 (not exported by software/bwamem.h) */
extern const bwtintv_v *smem_next2(smem_i *itr, int split_len, int split_width, int start_width);
/* defined in software/bwtindex.c:187 */
extern int bwa_index(int argc, char *argv[]);

static double now_s(void)
{
	struct timeval tv;
	gettimeofday(&tv, 0);
	return tv.tv_sec + tv.tv_usec * 1e-6;
}

typedef struct {
	int k, split_width, start_width;
	float split_factor;
} opts_t;

/* The seeding loop exactly as mem_chain()/mem_insert_seed() drive it. Emits
 * each returned list through cb (may be NULL). Returns number of calls. */
static int seed_one(const bwt_t *bwt, smem_i *itr, const opts_t *o, int len, const uint8_t *q,
		FILE *out, uint64_t *n_intv)
{
	const bwtintv_v *a;
	int n_calls = 0, split_len;
	long pos = 0;
	uint32_t zero = 0;
	if (out) { pos = ftell(out); fwrite(&zero, 4, 1, out); }
	if (len < o->k) goto done; /* software/bwamem.c:600 */
	split_len = (int)(o->k * o->split_factor + .499);
	split_len = split_len < len ? split_len : len;
	smem_set_query(itr, len, q);
	while ((a = smem_next2(itr, split_len, o->split_width, o->start_width)) != 0) {
		++n_calls;
		if (n_intv) *n_intv += a->n;
		if (out) {
			uint32_t n = (uint32_t)a->n;
			size_t i;
			fwrite(&n, 4, 1, out);
			for (i = 0; i < a->n; ++i) {
				uint64_t v[4] = { a->a[i].x[0], a->a[i].x[1], a->a[i].x[2], a->a[i].info };
				fwrite(v, 8, 4, out);
			}
		}
	}
done:
	if (out) {
		long end = ftell(out);
		uint32_t nc = (uint32_t)n_calls;
		fseek(out, pos, SEEK_SET);
		fwrite(&nc, 4, 1, out);
		fseek(out, end, SEEK_SET);
	}
	(void)bwt;
	return n_calls;
}

static int parse_opts(char **argv, opts_t *o)
{
	o->k = atoi(argv[0]);
	o->split_factor = (float)atof(argv[1]);
	o->split_width = atoi(argv[2]);
	o->start_width = atoi(argv[3]);
	return 0;
}

static int cmd_smem(int argc, char **argv)
{
	bwt_t *bwt;
	smrd_reads_t r;
	smem_i *itr;
	opts_t o;
	FILE *out;
	uint64_t i;
	if (argc < 8) { fprintf(stderr, "usage: smem <bwt> <reads> <out> <k> <r> <s> <start_width>\n"); return 1; }
	parse_opts(argv + 4, &o);
	bwt = bwt_restore_bwt(argv[1]);
	if (smrd_load(argv[2], &r) != 0) { fprintf(stderr, "cannot load reads %s\n", argv[2]); return 1; }
	out = fopen(argv[3], "wb");
	if (!out) return 1;
	smgo_write_header(out, r.n_reads);
	itr = smem_itr_init(bwt);
	for (i = 0; i < r.n_reads; ++i)
		seed_one(bwt, itr, &o, r.len[i], r.codes + r.off[i], out, 0);
	smem_itr_destroy(itr);
	fclose(out);
	smrd_free(&r);
	bwt_destroy(bwt);
	return 0;
}

typedef struct {
	const bwt_t *bwt;
	const smrd_reads_t *r;
	const opts_t *o;
	uint64_t beg, end, n_intv;
} bench_job_t;

static void *bench_worker(void *data)
{
	bench_job_t *j = (bench_job_t*)data;
	smem_i *itr = smem_itr_init(j->bwt);
	uint64_t i;
	for (i = j->beg; i < j->end; ++i)
		seed_one(j->bwt, itr, j->o, j->r->len[i], j->r->codes + j->r->off[i], 0, &j->n_intv);
	smem_itr_destroy(itr);
	return 0;
}

static int cmd_bench(int argc, char **argv)
{
	bwt_t *bwt;
	smrd_reads_t r;
	opts_t o;
	int t, n_threads;
	uint64_t n, n_intv = 0;
	double t0, t1;
	pthread_t *tid;
	bench_job_t *jobs;
	if (argc < 9) { fprintf(stderr, "usage: bench <bwt> <reads> <threads> <max_reads> <k> <r> <s> <sw>\n"); return 1; }
	parse_opts(argv + 5, &o);
	bwt = bwt_restore_bwt(argv[1]);
	if (smrd_load(argv[2], &r) != 0) return 1;
	n_threads = atoi(argv[3]);
	n = (uint64_t)atoll(argv[4]);
	if (n == 0 || n > r.n_reads) n = r.n_reads;
	tid = (pthread_t*)calloc(n_threads, sizeof(pthread_t));
	jobs = (bench_job_t*)calloc(n_threads, sizeof(bench_job_t));
	t0 = now_s();
	for (t = 0; t < n_threads; ++t) {
		jobs[t].bwt = bwt; jobs[t].r = &r; jobs[t].o = &o;
		jobs[t].beg = n * t / n_threads; jobs[t].end = n * (t + 1) / n_threads;
		pthread_create(&tid[t], 0, bench_worker, &jobs[t]);
	}
	for (t = 0; t < n_threads; ++t) { pthread_join(tid[t], 0); n_intv += jobs[t].n_intv; }
	t1 = now_s();
	printf("reads=%llu seconds=%.6f threads=%d reads_per_s=%.3f intervals=%llu\n",
			(unsigned long long)n, t1 - t0, n_threads, n / (t1 - t0), (unsigned long long)n_intv);
	free(tid); free(jobs); smrd_free(&r); bwt_destroy(bwt);
	return 0;
}

static int cmd_sa(int argc, char **argv)
{
	bwt_t *bwt;
	FILE *in, *out;
	char magic[8];
	uint64_t n_reads, r;
	int k, max_occ;
	if (argc < 7) { fprintf(stderr, "usage: sa <bwt> <sa> <in.smgo> <out.smsa> <k> <max_occ>\n"); return 1; }
	k = atoi(argv[5]);
	max_occ = atoi(argv[6]);
	bwt = bwt_restore_bwt(argv[1]);
	bwt_restore_sa(argv[2], bwt);
	in = fopen(argv[3], "rb");
	out = fopen(argv[4], "wb");
	if (!in || !out) return 1;
	if (fread(magic, 1, 8, in) != 8 || memcmp(magic, SMGO_MAGIC, 8) != 0) return 1;
	if (fread(&n_reads, 8, 1, in) != 1) return 1;
	smsa_write_header(out, n_reads);
	for (r = 0; r < n_reads; ++r) {
		uint32_t n_calls, c, n_occ = 0;
		long pos = ftell(out);
		if (fread(&n_calls, 4, 1, in) != 1) return 1;
		fwrite(&n_occ, 4, 1, out);
		for (c = 0; c < n_calls; ++c) {
			uint32_t n, i;
			if (fread(&n, 4, 1, in) != 1) return 1;
			for (i = 0; i < n; ++i) {
				uint64_t v[4];
				int slen;
				bwtint_t j;
				if (fread(v, 8, 4, in) != 4) return 1;
				slen = (uint32_t)v[3] - (int)(v[3] >> 32);
				if (slen < k || v[2] > (uint64_t)max_occ) continue;
				for (j = 0; j < v[2]; ++j) {
					uint64_t p = bwt_sa(bwt, v[0] + j);
					fwrite(&p, 8, 1, out);
					++n_occ;
				}
			}
		}
		{
			long end = ftell(out);
			fseek(out, pos, SEEK_SET);
			fwrite(&n_occ, 4, 1, out);
			fseek(out, end, SEEK_SET);
		}
	}
	fclose(in);
	fclose(out);
	bwt_destroy(bwt);
	return 0;
}

/* mem_seed_t / mem_chain_t / mem_chain_v are private to software/bwamem.c
 * (:317-327); these are layout-identical declarations to read its results */
typedef struct { int64_t rbeg; int32_t qbeg, len; } h_seed_t;
typedef struct { int n, m; int64_t pos; h_seed_t *seeds; } h_chain_t;
typedef struct { size_t n, m; h_chain_t *a; } h_chain_v;
extern h_chain_v mem_chain(const mem_opt_t *opt, const bwt_t *bwt, int64_t l_pac, int len, const uint8_t *seq);
extern int mem_chain_flt(const mem_opt_t *opt, int n_chn, h_chain_t *chains);

static int cmd_chain(int argc, char **argv)
{
	bwt_t *bwt;
	smrd_reads_t r;
	mem_opt_t *opt;
	FILE *out;
	uint64_t i;
	int filter;
	if (argc < 15) {
		fprintf(stderr, "usage: chain <bwt> <sa> <reads> <out> <k> <r> <s> <sw> <max_occ> <w> <gap> <mask> <drop> <filter>\n");
		return 1;
	}
	opt = mem_opt_init();
	opt->min_seed_len = atoi(argv[5]);
	opt->split_factor = (float)atof(argv[6]);
	opt->split_width = atoi(argv[7]);
	if (atoi(argv[8]) == 2) opt->flag |= MEM_F_NO_EXACT;
	opt->max_occ = atoi(argv[9]);
	opt->w = atoi(argv[10]);
	opt->max_chain_gap = atoi(argv[11]);
	opt->mask_level = (float)atof(argv[12]);
	opt->chain_drop_ratio = (float)atof(argv[13]);
	filter = atoi(argv[14]);
	bwt = bwt_restore_bwt(argv[1]);
	bwt_restore_sa(argv[2], bwt);
	if (smrd_load(argv[3], &r) != 0) return 1;
	out = fopen(argv[4], "wb");
	if (!out) return 1;
	smch_write_header(out, r.n_reads);
	for (i = 0; i < r.n_reads; ++i) {
		h_chain_v c = mem_chain(opt, bwt, (int64_t)(bwt->seq_len >> 1), r.len[i], r.codes + r.off[i]);
		uint32_t nc, j;
		if (filter) c.n = mem_chain_flt(opt, (int)c.n, c.a);
		nc = (uint32_t)c.n;
		fwrite(&nc, 4, 1, out);
		for (j = 0; j < nc; ++j) {
			uint32_t n = (uint32_t)c.a[j].n;
			int k;
			fwrite(&c.a[j].pos, 8, 1, out);
			fwrite(&n, 4, 1, out);
			for (k = 0; k < c.a[j].n; ++k) {
				fwrite(&c.a[j].seeds[k].rbeg, 8, 1, out);
				fwrite(&c.a[j].seeds[k].qbeg, 4, 1, out);
				fwrite(&c.a[j].seeds[k].len, 4, 1, out);
			}
		}
		for (j = 0; j < c.m && j < c.n; ++j) free(c.a[j].seeds);
		free(c.a);
	}
	fclose(out);
	smrd_free(&r);
	free(opt);
	bwt_destroy(bwt);
	return 0;
}

extern int mem_chain2aln_short(const mem_opt_t *opt, int64_t l_pac, const uint8_t *pac, int l_query,
		const uint8_t *query, const h_chain_t *c, mem_alnreg_v *av);
extern void mem_chain2aln(const mem_opt_t *opt, int64_t l_pac, const uint8_t *pac, int l_query, const uint8_t *query,
		const h_chain_t *c, mem_alnreg_v *av);

static int cmd_aln(int argc, char **argv)
{
	bwt_t *bwt;
	smrd_reads_t r;
	mem_opt_t *opt;
	FILE *out, *fp;
	uint64_t i;
	int64_t l_pac;
	uint8_t *pac;
	double t_aln = 0.0;
	uint64_t n_regs = 0;
	if (argc < 15) {
		fprintf(stderr, "usage: aln <bwt> <sa> <pac> <reads> <out> <k> <r> <s> <sw> <max_occ> <w> <gap> <mask> <drop>"
				" [a b o_del e_del o_ins e_ins zdrop pen_clip5 pen_clip3]\n");
		return 1;
	}
	if (argc != 15 && argc != 24) {
		fprintf(stderr, "aln: the scoring arguments come all nine or not at all\n");
		return 1;
	}
	opt = mem_opt_init();
	opt->min_seed_len = atoi(argv[6]);
	opt->split_factor = (float)atof(argv[7]);
	opt->split_width = atoi(argv[8]);
	if (atoi(argv[9]) == 2) opt->flag |= MEM_F_NO_EXACT;
	opt->max_occ = atoi(argv[10]);
	opt->w = atoi(argv[11]);
	opt->max_chain_gap = atoi(argv[12]);
	opt->mask_level = (float)atof(argv[13]);
	opt->chain_drop_ratio = (float)atof(argv[14]);
	if (argc == 24) {  /* literal values: no -A scaling of the others (software/fastmap.c:111-120) */
		opt->a = atoi(argv[15]); opt->b = atoi(argv[16]);
		opt->o_del = atoi(argv[17]); opt->e_del = atoi(argv[18]);
		opt->o_ins = atoi(argv[19]); opt->e_ins = atoi(argv[20]);
		opt->zdrop = atoi(argv[21]);
		opt->pen_clip5 = atoi(argv[22]); opt->pen_clip3 = atoi(argv[23]);
		bwa_fill_scmat(opt->a, opt->b, opt->mat);
	}
	bwt = bwt_restore_bwt(argv[1]);
	bwt_restore_sa(argv[2], bwt);
	l_pac = (int64_t)(bwt->seq_len >> 1);
	pac = calloc(l_pac / 4 + 1, 1);
	fp = fopen(argv[3], "rb");
	if (!fp || fread(pac, 1, (l_pac + 3) / 4, fp) != (size_t)((l_pac + 3) / 4)) return 1;
	fclose(fp);
	if (smrd_load(argv[4], &r) != 0) return 1;
	out = fopen(argv[5], "wb");
	if (!out) return 1;
	fwrite("SMRG0001", 1, 8, out);
	fwrite(&r.n_reads, 8, 1, out);
	for (i = 0; i < r.n_reads; ++i) {
		const uint8_t *q = r.codes + r.off[i];
		h_chain_v c = mem_chain(opt, bwt, l_pac, r.len[i], q);
		mem_alnreg_v av = { 0, 0, 0 };
		uint32_t j, n;
		c.n = mem_chain_flt(opt, (int)c.n, c.a);
		t_aln -= now_s();
		for (j = 0; j < c.n; ++j)   /* software/bwamem.c:1452-1460 */
			if (mem_chain2aln_short(opt, l_pac, pac, r.len[i], q, &c.a[j], &av) > 0)
				mem_chain2aln(opt, l_pac, pac, r.len[i], q, &c.a[j], &av);
		t_aln += now_s();
		n_regs += av.n;
		n = (uint32_t)av.n;
		fwrite(&n, 4, 1, out);
		for (j = 0; j < n; ++j) {
			const mem_alnreg_t *a = &av.a[j];
			int32_t v[10] = { a->qb, a->qe, a->score, a->truesc, a->sub, a->csub, a->sub_n, a->w, a->seedcov,
				a->secondary };
			fwrite(&a->rb, 8, 1, out);
			fwrite(&a->re, 8, 1, out);
			fwrite(v, 4, 10, out);
		}
		free(av.a);
		for (j = 0; j < c.m && j < c.n; ++j) free(c.a[j].seeds);
		free(c.a);
	}
	fclose(out);
	/* the chains -> regions loop alone, one thread: the alignment stage's CPU baseline */
	fprintf(stderr, "chain2aln_seconds=%.6f reads=%llu regions=%llu\n", t_aln, (unsigned long long)r.n_reads,
			(unsigned long long)n_regs);
	smrd_free(&r);
	free(pac);
	free(opt);
	bwt_destroy(bwt);
	return 0;
}

/* ksw <tasks.smkt> <out.smkr>: the reference's own ksw_extend2 on every task */
extern int ksw_extend2(int qlen, const uint8_t *query, int tlen, const uint8_t *target, int m, const int8_t *mat,
		int o_del, int e_del, int o_ins, int e_ins, int w, int end_bonus, int zdrop, int h0, int *_qle, int *_tle,
		int *_gtle, int *_gscore, int *_max_off);

typedef struct { uint64_t q_off, t_off; int32_t qlen, tlen, w, end_bonus, zdrop, h0; } ksw_task_t;

static int cmd_ksw(int argc, char **argv)
{
	char magic[8];
	uint64_t n, qb, tb, i;
	int8_t mat[28];
	int32_t pen[4];
	ksw_task_t *T;
	uint8_t *q, *t;
	FILE *fp, *out;
	if (argc < 3) { fprintf(stderr, "usage: ksw <tasks.smkt> <out.smkr>\n"); return 1; }
	fp = fopen(argv[1], "rb");
	if (!fp) return 1;
	if (fread(magic, 1, 8, fp) != 8 || memcmp(magic, SMKT_MAGIC, 8) != 0) return 1;
	if (fread(&n, 8, 1, fp) != 1 || fread(&qb, 8, 1, fp) != 1 || fread(&tb, 8, 1, fp) != 1) return 1;
	if (fread(mat, 1, 28, fp) != 28 || fread(pen, 4, 4, fp) != 4) return 1;
	T = malloc(sizeof(ksw_task_t) * (n ? n : 1));
	q = malloc(qb ? qb : 1);
	t = malloc(tb ? tb : 1);
	if (fread(T, sizeof(ksw_task_t), n, fp) != n || fread(q, 1, qb, fp) != qb || fread(t, 1, tb, fp) != tb) return 1;
	fclose(fp);
	out = fopen(argv[2], "wb");
	if (!out) return 1;
	fwrite(SMKR_MAGIC, 1, 8, out);
	fwrite(&n, 8, 1, out);
	for (i = 0; i < n; ++i) {
		int32_t r[6];
		r[0] = ksw_extend2(T[i].qlen, q + T[i].q_off, T[i].tlen, t + T[i].t_off, 5, mat, pen[0], pen[1], pen[2], pen[3],
				T[i].w, T[i].end_bonus, T[i].zdrop, T[i].h0, &r[1], &r[2], &r[3], &r[4], &r[5]);
		fwrite(r, 4, 6, out);
	}
	fclose(out);
	free(T); free(q); free(t);
	return 0;
}

typedef struct { uint64_t q_off, t_off; int32_t qlen, tlen, xtra, pad; } kswa_task_t;

static int cmd_kswa(int argc, char **argv)
{
	char magic[8];
	uint64_t n, qb, tb, i;
	int8_t mat[28];
	int32_t pen[4];
	kswa_task_t *T;
	uint8_t *q, *t;
	FILE *fp, *out;
	if (argc < 3) { fprintf(stderr, "usage: kswa <tasks.smat> <out.smar>\n"); return 1; }
	fp = fopen(argv[1], "rb");
	if (!fp) return 1;
	if (fread(magic, 1, 8, fp) != 8 || memcmp(magic, "SMAT0001", 8) != 0) return 1;
	if (fread(&n, 8, 1, fp) != 1 || fread(&qb, 8, 1, fp) != 1 || fread(&tb, 8, 1, fp) != 1) return 1;
	if (fread(mat, 1, 28, fp) != 28 || fread(pen, 4, 4, fp) != 4) return 1;
	T = malloc(sizeof(kswa_task_t) * (n ? n : 1));
	q = malloc(qb ? qb : 1);
	t = malloc(tb ? tb : 1);
	if (fread(T, sizeof(kswa_task_t), n, fp) != n || fread(q, 1, qb, fp) != qb || fread(t, 1, tb, fp) != tb) return 1;
	fclose(fp);
	out = fopen(argv[2], "wb");
	if (!out) return 1;
	fwrite("SMAR0001", 1, 8, out);
	fwrite(&n, 8, 1, out);
	for (i = 0; i < n; ++i) {
		kswr_t r = ksw_align2(T[i].qlen, q + T[i].q_off, T[i].tlen, t + T[i].t_off, 5, mat, pen[0], pen[1], pen[2], pen[3],
				T[i].xtra, 0);
		int32_t v[7] = { r.score, r.te, r.qe, r.score2, r.te2, r.tb, r.qb };
		fwrite(v, 4, 7, out);
	}
	fclose(out);
	free(T); free(q); free(t);
	return 0;
}

/* msw <in.smmi> <out.smmo>: the reference's own mem_matesw on given lists */
extern int mem_matesw(const mem_opt_t *opt, int64_t l_pac, const uint8_t *pac, const mem_pestat_t pes[4],
		const mem_alnreg_t *a, int l_ms, const uint8_t *ms, mem_alnreg_v *ma);

/* a region as the files hold it: the fields of tests/regfin_ref.py's FIELDS, 64 bytes */
typedef struct { int64_t rb, re; int32_t v[10]; uint64_t hash; } msw_reg_t;

static void msw_to_ref(const msw_reg_t *s, mem_alnreg_t *d)
{
	memset(d, 0, sizeof(*d));
	d->rb = s->rb; d->re = s->re;
	d->qb = s->v[0]; d->qe = s->v[1]; d->score = s->v[2]; d->truesc = s->v[3]; d->sub = s->v[4]; d->csub = s->v[5];
	d->sub_n = s->v[6]; d->w = s->v[7]; d->seedcov = s->v[8]; d->secondary = s->v[9];
	d->hash = s->hash;
}

static void msw_from_ref(const mem_alnreg_t *a, msw_reg_t *d)
{
	int32_t v[10] = { a->qb, a->qe, a->score, a->truesc, a->sub, a->csub, a->sub_n, a->w, a->seedcov, a->secondary };
	d->rb = a->rb; d->re = a->re;
	memcpy(d->v, v, sizeof(v));
	d->hash = a->hash;
}

static int cmd_msw(int argc, char **argv)
{
	char magic[8];
	int64_t l_pac;
	int32_t pe[12], o[10];
	float mask_level_redun;
	uint64_t cnt[4], n_pairs, n_pac, n_codes, n_regs, p, n_out = 0, m_out = 0;
	uint8_t *pac, *codes;
	uint64_t *offs, *reg_off, *out_off;
	msw_reg_t *regs, *out = 0;
	int32_t *n_sw;
	mem_opt_t *opt;
	mem_pestat_t pes[4];
	FILE *fp;
	int r;
	if (argc < 3) { fprintf(stderr, "usage: msw <in.smmi> <out.smmo>\n"); return 1; }
	fp = fopen(argv[1], "rb");
	if (!fp) return 1;
	if (fread(magic, 1, 8, fp) != 8 || memcmp(magic, "SMMI0001", 8) != 0) return 1;
	if (fread(&l_pac, 8, 1, fp) != 1 || fread(pe, 4, 12, fp) != 12 || fread(o, 4, 10, fp) != 10) return 1;
	if (fread(&mask_level_redun, 4, 1, fp) != 1 || fread(cnt, 8, 4, fp) != 4) return 1;
	n_pairs = cnt[0]; n_pac = cnt[1]; n_codes = cnt[2]; n_regs = cnt[3];
	if (l_pac < 1 || n_pac < (uint64_t)(l_pac + 3) / 4) return 1;
	pac = calloc(n_pac + 1, 1);
	codes = malloc(n_codes ? n_codes : 1);
	offs = malloc(8 * (2 * n_pairs + 1));
	reg_off = malloc(8 * (2 * n_pairs + 1));
	out_off = malloc(8 * (2 * n_pairs + 1));
	regs = malloc(sizeof(msw_reg_t) * (n_regs ? n_regs : 1));
	n_sw = malloc(4 * (n_pairs ? n_pairs : 1));
	if (fread(pac, 1, n_pac, fp) != n_pac || fread(codes, 1, n_codes, fp) != n_codes) return 1;
	if (fread(offs, 8, 2 * n_pairs + 1, fp) != 2 * n_pairs + 1) return 1;
	if (fread(reg_off, 8, 2 * n_pairs + 1, fp) != 2 * n_pairs + 1) return 1;
	if (fread(regs, sizeof(msw_reg_t), n_regs, fp) != n_regs) return 1;
	fclose(fp);
	if (offs[2 * n_pairs] > n_codes || reg_off[2 * n_pairs] > n_regs) return 1;
	opt = mem_opt_init();
	opt->a = o[0]; opt->b = o[1];
	opt->o_del = o[2]; opt->e_del = o[3]; opt->o_ins = o[4]; opt->e_ins = o[5];
	opt->min_seed_len = o[6]; opt->pen_unpaired = o[7]; opt->max_matesw = o[8];
	opt->mask_level_redun = mask_level_redun;
	bwa_fill_scmat(opt->a, opt->b, opt->mat);
	memset(pes, 0, sizeof(pes));
	for (r = 0; r < 4; ++r) pes[r].low = pe[3 * r], pes[r].high = pe[3 * r + 1], pes[r].failed = pe[3 * r + 2];
	out_off[0] = 0;
	for (p = 0; p < n_pairs; ++p) {
		mem_alnreg_v a[2], b[2];
		int e, j, n = 0;
		for (e = 0; e < 2; ++e) {   /* the pair's lists, and of each the good hits as they came */
			uint64_t lo = reg_off[2 * p + e], k, cnt_e = reg_off[2 * p + e + 1] - lo;
			a[e].n = a[e].m = cnt_e; a[e].a = malloc(sizeof(mem_alnreg_t) * (cnt_e ? cnt_e : 1));
			b[e].n = 0; b[e].m = cnt_e; b[e].a = malloc(sizeof(mem_alnreg_t) * (cnt_e ? cnt_e : 1));
			for (k = 0; k < cnt_e; ++k) msw_to_ref(&regs[lo + k], &a[e].a[k]);
			for (k = 0; k < cnt_e; ++k)
				if (a[e].a[k].score >= a[e].a[0].score - opt->pen_unpaired) b[e].a[b[e].n++] = a[e].a[k];
		}
		for (e = 0; e < 2; ++e) {   /* end e's hits rescue the other end, end 0's first */
			const int m = 1 - e;
			for (j = 0; j < (int)b[e].n && j < opt->max_matesw; ++j)
				n += mem_matesw(opt, l_pac, pac, pes, &b[e].a[j], (int)(offs[2 * p + m + 1] - offs[2 * p + m]),
						codes + offs[2 * p + m], &a[m]);
		}
		n_sw[p] = n;
		for (e = 0; e < 2; ++e) {
			uint64_t k;
			if (n_out + a[e].n > m_out) {
				m_out = (n_out + a[e].n) * 2 + 16;
				out = realloc(out, sizeof(msw_reg_t) * m_out);
			}
			for (k = 0; k < a[e].n; ++k) msw_from_ref(&a[e].a[k], &out[n_out + k]);
			n_out += a[e].n;
			out_off[2 * p + e + 1] = n_out;
			free(a[e].a); free(b[e].a);
		}
	}
	fp = fopen(argv[2], "wb");
	if (!fp) return 1;
	fwrite("SMMO0001", 1, 8, fp);
	fwrite(&n_pairs, 8, 1, fp);
	fwrite(&n_out, 8, 1, fp);
	fwrite(n_sw, 4, n_pairs, fp);
	fwrite(out_off, 8, 2 * n_pairs + 1, fp);
	fwrite(out, sizeof(msw_reg_t), n_out, fp);
	fclose(fp);
	free(pac); free(codes); free(offs); free(reg_off); free(out_off); free(regs); free(n_sw); free(out); free(opt);
	return 0;
}

/* the HARP-path globals of software/fastmap.c:27-29 and software/main.c:28 (their
 * definitions are linked from the reference objects; allocated here as
 * main_mem and the manager thread do) */
extern unsigned long int **worker_mem;
extern volatile unsigned char *sw_handshake;
extern char *bwa_pg;

/* `bwa mem`'s scoring options as main_mem reads them (software/fastmap.c:54-94,
 * 159-171): -k -w -A -B -O -E -L -d, INT or INT,INT where bwa takes a pair; -A
 * scales the penalties, T, zdrop and the clip penalties that were not given */
static int pair_arg(const char *s, int *x, int *y)
{
	char *p;
	*x = *y = (int)strtol(s, &p, 10);
	if (*p == ',' && p[1] >= '0' && p[1] <= '9') *y = (int)strtol(p + 1, &p, 10);
	return *p == 0 ? 0 : -1;
}

static int mem_options(mem_opt_t *opt, int n, char **av)
{
	int i, set_a = 0, set_b = 0, set_o = 0, set_e = 0, set_l = 0, set_d = 0;
	if (n & 1) return -1;
	for (i = 0; i < n; i += 2) {
		const char *k = av[i], *v = av[i + 1];
		if (k[0] != '-' || k[1] == 0 || k[2] != 0) return -1;
		switch (k[1]) {
		case 'k': opt->min_seed_len = atoi(v); break;
		case 'w': opt->w = atoi(v); break;
		case 'A': opt->a = atoi(v); set_a = 1; break;
		case 'B': opt->b = atoi(v); set_b = 1; break;
		case 'd': opt->zdrop = atoi(v); set_d = 1; break;
		case 'O': if (pair_arg(v, &opt->o_del, &opt->o_ins)) return -1; set_o = 1; break;
		case 'E': if (pair_arg(v, &opt->e_del, &opt->e_ins)) return -1; set_e = 1; break;
		case 'L': if (pair_arg(v, &opt->pen_clip5, &opt->pen_clip3)) return -1; set_l = 1; break;
		default: return -1;
		}
	}
	if (set_a) {
		if (!set_b) opt->b *= opt->a;
		opt->T *= opt->a;
		if (!set_o) opt->o_del *= opt->a, opt->o_ins *= opt->a;
		if (!set_e) opt->e_del *= opt->a, opt->e_ins *= opt->a;
		if (!set_d) opt->zdrop *= opt->a;
		if (!set_l) opt->pen_clip5 *= opt->a, opt->pen_clip3 *= opt->a;
		opt->pen_unpaired *= opt->a;
	}
	bwa_fill_scmat(opt->a, opt->b, opt->mat);
	return 0;
}

static int cmd_mem(int argc, char **argv)
{
	mem_opt_t *opt;
	bwt_t *bwt;
	bntseq_t *bns;
	uint8_t *pac;
	char *tmp;
	gzFile fp;
	kseq_t *ks;
	bseq1_t *seqs;
	int i, n;
	int64_t n_processed = 0;
	if (argc < 6) {
		fprintf(stderr, "usage: mem <prefix> <reads.fq> <threads> <batch> <pe> [pg [-k|-w|-A|-B|-O|-E|-L|-d VALUE]...]\n");
		return 1;
	}
	opt = mem_opt_init();
	opt->n_threads = atoi(argv[3]);
	opt->batch_size = atoi(argv[4]) > 1? atoi(argv[4]) : 1;
	if (atoi(argv[5])) opt->flag |= MEM_F_PE;
	bwa_pg = argc > 6? argv[6] : "@PG\tID:bwa\tPN:bwa\tVN:0.7.8-r455";
	if (argc > 7 && mem_options(opt, argc - 7, argv + 7) != 0) {
		fprintf(stderr, "mem: bad option list\n");
		return 1;
	}
	tmp = calloc(strlen(argv[1]) + 5, 1);
	strcat(strcpy(tmp, argv[1]), ".bwt");
	bwt = bwt_restore_bwt(tmp);
	strcat(strcpy(tmp, argv[1]), ".sa");
	bwt_restore_sa(tmp, bwt);
	free(tmp);
	bns = bns_restore(argv[1]);
	pac = calloc(bns->l_pac / 4 + 1, 1);
	err_fread_noeof(pac, 1, bns->l_pac / 4 + 1, bns->fp_pac);
	err_fclose(bns->fp_pac);
	bns->fp_pac = 0;
	fp = gzopen(argv[2], "r");
	if (!fp) return 1;
	ks = kseq_init(fp);
	bwa_print_sam_hdr(bns, 0);
	worker_mem = (unsigned long int **)malloc(sizeof(unsigned long int *) * opt->n_threads);
	for (i = 0; i < opt->n_threads; ++i)
		worker_mem[i] = (unsigned long int *)malloc(sizeof(unsigned long int) * 1024 * 1024 + 1);
	sw_handshake = (unsigned char *)calloc(opt->n_threads + 1, 1);
	while ((seqs = bseq_read(opt->chunk_size * opt->n_threads, &n, ks, 0)) != 0) {
		if ((opt->flag & MEM_F_PE) && (n & 1)) n = n >> 1 << 1;
		for (i = 0; i < n; ++i) { free(seqs[i].comment); seqs[i].comment = 0; }
		mem_process_seqs(opt, bwt, bns, pac, n_processed, n, seqs, 0);
		n_processed += n;
		for (i = 0; i < n; ++i) {
			err_fputs(seqs[i].sam, stdout);
			free(seqs[i].name); free(seqs[i].comment); free(seqs[i].seq); free(seqs[i].qual); free(seqs[i].sam);
		}
		free(seqs);
	}
	for (i = 0; i < opt->n_threads; ++i) free(worker_mem[i]);
	free(worker_mem);
	free((void*)sw_handshake);
	kseq_destroy(ks);
	gzclose(fp);
	free(pac);
	bns_destroy(bns);
	bwt_destroy(bwt);
	free(opt);
	fflush(stdout);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc < 2) {
		fprintf(stderr, "usage: ref_harness index|smem|bench|sa ...\n");
		return 1;
	}
	if (strcmp(argv[1], "index") == 0) {
		char *av[7];
		if (argc < 4) return 1;
		av[0] = "index"; av[1] = "-a"; av[2] = "is"; av[3] = "-p"; av[4] = argv[3]; av[5] = argv[2]; av[6] = 0;
		return bwa_index(6, av);
	}
	if (strcmp(argv[1], "smem") == 0) return cmd_smem(argc - 1, argv + 1);
	if (strcmp(argv[1], "bench") == 0) return cmd_bench(argc - 1, argv + 1);
	if (strcmp(argv[1], "sa") == 0) return cmd_sa(argc - 1, argv + 1);
	if (strcmp(argv[1], "chain") == 0) return cmd_chain(argc - 1, argv + 1);
	if (strcmp(argv[1], "ksw") == 0) return cmd_ksw(argc - 1, argv + 1);
	if (strcmp(argv[1], "aln") == 0) return cmd_aln(argc - 1, argv + 1);
	if (strcmp(argv[1], "mem") == 0) return cmd_mem(argc - 1, argv + 1);
	if (strcmp(argv[1], "kswa") == 0) return cmd_kswa(argc - 1, argv + 1);
	if (strcmp(argv[1], "msw") == 0) return cmd_msw(argc - 1, argv + 1);
	fprintf(stderr, "unknown command %s\n", argv[1]);
	return 1;
}
