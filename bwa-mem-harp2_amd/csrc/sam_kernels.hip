// Alignments -> SAM text (csrc/sam_kernels.h), single-end and paired-end: a length pass (one lane per record,
// then one lane per read), the offset scan of smem_kernels.hip over the reads' byte counts, and
// a write pass, one wave per read: the wave assembles the read's lines in an LDS window that
// follows the output stream 16 bytes at a time and stores every whole 16-byte chunk with one
// dwordx4 store per lane; only the bytes before the first and after the last 16-byte boundary
// of a read's text (they share their chunk with a neighbouring read's text) are stored singly.
// The paired-end text has kernels of its own (sam_len_pe_kernel, sam_read_pe_kernel,
// sam_write_pe_kernel) over the same helpers: every line also carries what mem_aln2sam takes
// from the mate, record 0 of the pair's other read.
#include "sam_kernels.h"

namespace smem {
namespace {

// ---- numbers as kputw / kputl print them (software/kstring.h)
__device__ inline uint32_t ndig32(uint32_t v) {
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) +
           (v >= 10000000u) + (v >= 100000000u) + (v >= 1000000000u);
}
__device__ inline uint32_t ndig64(uint64_t v) {
    if (v <= 0xffffffffull) return ndig32((uint32_t)v);
    uint32_t n = 0;
    while (v) v /= 10, ++n;
    return n;
}
__device__ inline uint32_t num_len(int64_t v) {
    return v < 0 ? 1u + ndig64(0ull - (uint64_t)v) : ndig64((uint64_t)v);
}
// character i of the decimal form of v (num_len(v) characters)
__device__ inline char num_char(int64_t v, uint32_t len, uint32_t i) {
    const bool neg = v < 0;
    if (neg && i == 0) return '-';
    const uint64_t m = neg ? 0ull - (uint64_t)v : (uint64_t)v;
    uint32_t drop = len - 1 - i;  // digits to the right of this one
    if (m <= 0xffffffffull) {
        uint32_t x = (uint32_t)m;
        while (drop--) x /= 10u;
        return (char)('0' + x % 10u);
    }
    uint64_t x = m;
    while (drop--) x /= 10ull;
    return (char)('0' + (uint32_t)(x % 10ull));
}

// "MIDSH"[op] with clips as S (hard 0) or H (hard 1): software/bwamem.c:1240-1242, 1317
__device__ inline char cigar_letter(uint32_t op, int hard) {
    if (op == 3 || op == 4) op = hard ? 4 : 3;
    return (char)((0x485344494Dull >> (8 * (op > 4 ? 4 : op))) & 0xff);
}
// "ACGTN"[c] / "TGCAN"[c] (software/bwamem.c:1273, 1287)
__device__ inline char base_fwd(uint32_t c) { return (char)((0x4E54474341ull >> (8 * (c > 4 ? 4 : c))) & 0xff); }
__device__ inline char base_rev(uint32_t c) { return (char)((0x4E41434754ull >> (8 * (c > 4 ? 4 : c))) & 0xff); }

// bytes of a CIGAR's text: a number and a letter per word
__device__ inline uint32_t cigar_len(const uint32_t* w, int n) {
    uint32_t len = 0;
    for (int i = 0; i < n; ++i) len += ndig32(w[i] >> 4) + 1;
    return len;
}

// the fields of record k that finalize decided
struct RecV {
    int32_t mapq, flag, score, xs;
};
__device__ inline RecV rec_of(const SamParams& P, uint64_t k) {
    if (P.recs) {
        const SamRec s = P.recs[k];
        return RecV{s.mapq, s.flag, s.score, s.xs};
    }
    const uint64_t j = P.idx[k];
    const FinSel s = P.sel[j];
    return RecV{s.mapq, s.flag, P.regs[j].score, s.xs};
}

// the read's [qb, qe) a record prints: clips are trimmed from every record but the first, and on
// the reverse strand cigar[0] trims the end and the last word the start (software/bwamem.c:1267-1271,
// 1281-1285)
__device__ inline void seq_range(const uint32_t* cg, int n_cigar, int which, int is_rev, int l_seq, int* qb, int* qe) {
    int b = 0, e = l_seq;
    if (n_cigar > 0 && which) {
        const uint32_t w0 = cg[0], w1 = cg[n_cigar - 1];
        const int first = ((w0 & 0xf) == 3 || (w0 & 0xf) == 4) ? (int)(w0 >> 4) : 0;
        const int last = ((w1 & 0xf) == 3 || (w1 & 0xf) == 4) ? (int)(w1 >> 4) : 0;
        if (!is_rev) b += first, e -= last;
        else e -= first, b += last;
    }
    if (b < 0) b = 0;
    if (e > l_seq) e = l_seq;
    if (e < b) e = b;
    *qb = b, *qe = e;
}

__device__ inline uint32_t name_len_of(const SamParams& P, uint32_t r) { return (uint32_t)(P.name_off[r + 1] - P.name_off[r]); }
__device__ inline uint32_t comment_len_of(const SamParams& P, uint32_t r) {
    return P.comments ? (uint32_t)(P.comment_off[r + 1] - P.comment_off[r]) : 0u;
}
__device__ inline uint32_t ctg_name_len(const SamParams& P, int rid) {
    return (uint32_t)(P.ctg_name_off[rid + 1] - P.ctg_name_off[rid]);
}
// the tags every line of a read ends with, and its newline (software/bwamem.c:1303, 1325-1326)
__device__ inline uint32_t tail_len(const SamParams& P, uint32_t r) {
    const uint32_t cl = comment_len_of(P, r);
    return (P.rg_len ? 6u + P.rg_len : 0u) + (cl ? 1u + cl : 0u) + 1u;
}

// ---- the length pass
// get_rlen (software/bwamem.c:1203-1212): the M and D lengths of a CIGAR, an int as the reference's
__device__ inline int cigar_rlen(const uint32_t* w, int n) {
    int l = 0;
    for (int i = 0; i < n; ++i) {
        const uint32_t op = w[i] & 0xf;
        if (op == 0 || op == 2) l += (int)(w[i] >> 4);
    }
    return l;
}

// one lane per record.  PE (the paired-end text): the record's MAPQ is the pair's in branch 1 and
// 2, its reference length is kept, and the bytes of FLAG, RNEXT, PNEXT and TLEN -- they depend on
// the mate's record -- are left to sam_read_pe_kernel
template <bool PE>
__device__ __forceinline__ void sam_len_record(const SamParams& P, const SamPair* pairs, uint32_t* rlen) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= P.n_rec) return;
    // the read of record k: rec_off[r] <= k < rec_off[r + 1]
    uint32_t lo = 0, hi = P.n_reads;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (P.rec_off[mid + 1] <= k) lo = mid + 1;
        else hi = mid;
    }
    const uint32_t r = lo;
    const Aln A = P.alns[k];
    RecV V = rec_of(P, k);
    if (PE) {
        const SamPair S = pairs[r >> 1];
        if (S.mode > 0) V.mapq = (r & 1u) ? S.mapq[1] : S.mapq[0];   // h[e].mapq = q_se[e] (software/bwamem_pair.c:306-307)
    }
    const int rid = P.rid[k];
    if (A.status != 0 || V.mapq == -1 || rid < 0 || rid >= P.n_ctg || A.n_cigar < 0) {
        P.rec_len[k] = 1u << 31;   // the read is the host's
        P.sa_len[k] = 0;
        if (PE) rlen[k] = 0;
        return;
    }
    const int which = (int)(k - P.rec_off[r]);
    const int l_seq = (int)(P.offs[r + 1] - P.offs[r]);
    const uint32_t* cg = P.cigar + A.cigar_off;
    const uint32_t cl = A.n_cigar ? cigar_len(cg, A.n_cigar) : 1u;
    const int flag = V.flag | (A.is_rev ? 0x10 : 0);
    const int64_t pos1 = A.pos - P.ctg_off[rid] + 1;
    const uint32_t coord = ctg_name_len(P, rid) + 1 + num_len(pos1) + 1;
    uint32_t len = name_len_of(P, r) + 1 + (PE ? 0u : num_len((flag & 0xffff) | (flag & 0x10000 ? 0x100 : 0))) + 1;
    len += coord + num_len(V.mapq) + 1 + cl;
    len += 1 + (PE ? 0u : 5u) + 1;                  // the mate fields
    if (PE) rlen[k] = (uint32_t)cigar_rlen(cg, A.n_cigar);
    if (flag & 0x100) {
        len += 3;
    } else {
        int qb, qe;
        seq_range(cg, A.n_cigar, which, A.is_rev, l_seq, &qb, &qe);
        len += (uint32_t)(qe - qb) + 1 + (P.qual ? (uint32_t)(qe - qb) : 1u);
    }
    if (A.n_cigar) len += 6 + num_len(A.NM) + 6 + (uint32_t)A.md_len;
    if (V.score >= 0) len += 6 + num_len(V.score);
    if (V.xs >= 0) len += 6 + num_len(V.xs);
    len += tail_len(P, r);
    P.rec_len[k] = len & 0x7fffffffu;
    // rname,pos,strand,CIGAR,mapq,NM; -- 0 marks a record no SA:Z lists (software/bwamem.c:1312)
    P.sa_len[k] = (flag & 0x100) ? 0u : coord + 2 + cl + 1 + num_len(V.mapq) + 1 + num_len(A.NM) + 1;
}

__global__ __launch_bounds__(256) void sam_len_kernel(SamParams P) { sam_len_record<false>(P, nullptr, nullptr); }
__global__ __launch_bounds__(256) void sam_len_pe_kernel(SamPeParams X) { sam_len_record<true>(X.s, X.pairs, X.rlen); }

// bytes of the unmapped line (software/bwamem.c:1381-1385: rid -1, flag 4, AS:i:0, XS:i:0)
__device__ inline uint64_t unmapped_len(const SamParams& P, uint32_t r) {
    const uint64_t l_seq = P.offs[r + 1] - P.offs[r];
    return name_len_of(P, r) + 1 + 1 + 1 + 7 + 1 + 5 + 1 + l_seq + 1 + (P.qual ? l_seq : 1) + 7 + 7 + tail_len(P, r);
}

__global__ __launch_bounds__(256) void sam_read_kernel(SamParams P) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= P.n_reads) return;
    const uint64_t lo = P.rec_off[r], hi = P.rec_off[r + 1];
    bool host = (P.fin_status && P.fin_status[r] == FIN_REJECT) || P.offs[r + 1] == P.offs[r];
    uint64_t tot = 0, sum_sa = 0, n_prim = 0;
    for (uint64_t k = lo; k < hi; ++k) {
        const uint32_t rl = P.rec_len[k], sl = P.sa_len[k];
        host |= (rl >> 31) != 0;
        tot += rl & 0x7fffffffu;
        if (sl) n_prim += 1, sum_sa += sl;
    }
    // every record an SA:Z lists also prints one: "\tSA:Z:" and the other records' entries
    if (n_prim >= 2) tot += n_prim * 6 + (n_prim - 1) * sum_sa;
    if (lo == hi) tot = unmapped_len(P, r);
    P.read_bytes[r] = host ? 0 : tot;
    P.status[r] = host ? SAM_HOST : 0;
    if (host) atomicAdd(P.cnt + SAM_N_HOST, 1u);
}

// ---- the paired-end lines: mem_aln2sam with a mate (software/bwamem.c:1219-1260)
// the mate of every line of read r: record 0 of read r ^ 1 (h[!e], software/bwamem_pair.c:306-307,
// 316-320), or none for a read without a record (mem_reg2aln(.., 0): rid -1)
struct Mate {
    bool has;
    int rid, is_rev, n_cigar, rlen;
    int64_t pos;
};
__device__ __forceinline__ Mate mate_of(const SamPeParams& X, uint32_t r) {
    const SamParams& P = X.s;
    const uint64_t lo = P.rec_off[r ^ 1u], hi = P.rec_off[(r ^ 1u) + 1];
    Mate M{hi > lo, -1, 0, 0, 0, -1};
    if (M.has) {
        const Aln A = P.alns[lo];
        M.rid = P.rid[lo], M.is_rev = A.is_rev, M.n_cigar = A.n_cigar, M.rlen = (int)X.rlen[lo], M.pos = A.pos;
    }
    return M;
}
// extra_flag & 2 of read r's lines: the pair's own in branch 1 and 2; in branch 0 the test of
// :324-325 counts only where h[0].rid == h[1].rid >= 0 (software/bwamem_pair.c:321)
__device__ __forceinline__ int proper_of(const SamPeParams& X, uint32_t r, const Mate& M) {
    const SamPair S = X.pairs[r >> 1];
    if (!S.proper) return 0;
    if (S.mode != 0) return 2;
    const uint64_t lo = X.s.rec_off[r];
    return lo < X.s.rec_off[r + 1] && M.has && X.s.rid[lo] == M.rid ? 2 : 0;
}

// what a line owes to the pair: its FLAG, and RNEXT (rid of the name; eq: '='; rid < 0: "*\t0\t0"),
// PNEXT, TLEN
struct PeLine {
    int flag, mrid;
    bool eq;
    int64_t pnext, tlen;
};
// a record's line (software/bwamem.c:1221-1229, 1249-1260); vflag is the record's own flag
__device__ __forceinline__ PeLine pe_line(const SamParams& P, uint32_t r, const Mate& M, int proper, int vflag, int rid,
                                          const Aln& A, int rlen) {
    PeLine L;
    L.flag = vflag | 0x1 | (0x40 << (r & 1u)) | proper | (A.is_rev ? 0x10 : 0);
    L.tlen = 0;
    if (M.has) {
        L.flag |= M.is_rev ? 0x20 : 0;
        L.mrid = M.rid, L.eq = rid == M.rid, L.pnext = M.pos - P.ctg_off[M.rid] + 1;
        if (L.eq && A.n_cigar != 0 && M.n_cigar != 0) {                                       // :1254-1258
            const int64_t p0 = A.pos + (A.is_rev ? rlen - 1 : 0), p1 = M.pos + (M.is_rev ? M.rlen - 1 : 0);
            L.tlen = -(p0 - p1 + (p0 > p1 ? 1 : p0 < p1 ? -1 : 0));
        }
    } else {  // copy alignment to mate (:1226-1227)
        L.flag |= 0x8 | (A.is_rev ? 0x20 : 0);
        L.mrid = rid, L.eq = true, L.pnext = A.pos - P.ctg_off[rid] + 1;
    }
    return L;
}
// the line of a read without a record: with a mapped mate it takes the mate's coordinate and
// strand (copy mate to alignment, :1224-1225)
__device__ __forceinline__ PeLine pe_line_unmapped(const SamParams& P, uint32_t r, const Mate& M) {
    PeLine L;
    L.flag = 0x4 | 0x1 | (0x40 << (r & 1u));
    L.tlen = 0, L.eq = true, L.mrid = -1, L.pnext = 0;
    if (M.has) {
        L.flag |= M.is_rev ? 0x30 : 0;
        L.mrid = M.rid, L.pnext = M.pos - P.ctg_off[M.rid] + 1;
    } else {
        L.flag |= 0x8;
    }
    return L;
}
__device__ __forceinline__ uint32_t flag_len(int flag) { return num_len((flag & 0xffff) | (flag & 0x10000 ? 0x100 : 0)); }
// bytes of RNEXT, PNEXT and TLEN with the two tabs between them
__device__ __forceinline__ uint32_t mate_len(const SamParams& P, const PeLine& L) {
    if (L.mrid < 0) return 5;
    return (L.eq ? 1u : ctg_name_len(P, L.mrid)) + 1 + num_len(L.pnext) + 1 + num_len(L.tlen);
}

// one lane per read: the pair is the host's when either read is; a record's line adds its FLAG
// and mate fields; a read without a record prints the unmapped line or the placed one
__global__ __launch_bounds__(256) void sam_read_pe_kernel(SamPeParams X) {
    const SamParams& P = X.s;
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= P.n_reads) return;
    const uint64_t lo = P.rec_off[r], hi = P.rec_off[r + 1];
    bool host = X.pairs[r >> 1].mode < 0;
    for (uint32_t q = r & ~1u; q <= (r | 1u); ++q) {
        host |= (P.fin_status && P.fin_status[q] == FIN_REJECT) || P.offs[q + 1] == P.offs[q];
        for (uint64_t k = P.rec_off[q]; k < P.rec_off[q + 1]; ++k) host |= (P.rec_len[k] >> 31) != 0;
    }
    uint64_t tot = 0;
    if (!host) {  // (only now is every record of the pair known to have a contig)
        const Mate M = mate_of(X, r);
        if (lo == hi) {
            const PeLine L = pe_line_unmapped(P, r, M);
            const uint64_t l_seq = P.offs[r + 1] - P.offs[r];
            const uint32_t coord = M.has ? ctg_name_len(P, M.rid) + 1 + num_len(L.pnext) + 4 : 7u;   // RNAME POS 0 *
            tot = name_len_of(P, r) + 1 + flag_len(L.flag) + 1 + coord + 1 + mate_len(P, L) + 1 + l_seq + 1 +
                  (P.qual ? l_seq : 1) + 7 + 7 + tail_len(P, r);
        } else {
            const int proper = proper_of(X, r, M);
            uint64_t sum_sa = 0, n_prim = 0;
            for (uint64_t k = lo; k < hi; ++k) {
                const uint32_t sl = P.sa_len[k];
                const PeLine L = pe_line(P, r, M, proper, rec_of(P, k).flag, P.rid[k], P.alns[k], (int)X.rlen[k]);
                tot += (P.rec_len[k] & 0x7fffffffu) + flag_len(L.flag) + mate_len(P, L);
                if (sl) n_prim += 1, sum_sa += sl;
            }
            if (n_prim >= 2) tot += n_prim * 6 + (n_prim - 1) * sum_sa;
        }
    }
    P.read_bytes[r] = tot;
    P.status[r] = host ? SAM_HOST : 0;
    if (host) atomicAdd(P.cnt + SAM_N_HOST, 1u);
}

// ---- the write pass
// A wave's window onto the output: lds[0, fill) holds text[base, base + fill), base a multiple
// of 16; the first `skip` bytes lie before the read's text and are never stored.  Every member
// is the same in all lanes.
__shared__ __attribute__((aligned(16))) char lds[SAM_BUF];

#define SAM_INLINE __device__ __forceinline__

struct Out {
    char* text;
    uint64_t base, end;
    uint32_t fill, skip;
    bool over;  // the read's lines did not fit its counted bytes (the staging stops at `end`)

    SAM_INLINE void flush(bool final) {
        const uint32_t lane = threadIdx.x;
        __syncthreads();
        const uint32_t n_chunks = fill >> 4, body = fill & ~15u, rem = fill & 15u;
        // with a head, chunk 0 shares its 16 bytes with the text before the read's
        if (n_chunks && skip && lane >= skip && lane < 16) text[base + lane] = lds[lane];
        for (uint32_t c = (skip ? 1u : 0u) + lane; c < n_chunks; c += 64)
            *reinterpret_cast<uint4*>(text + base + 16ull * c) = *reinterpret_cast<const uint4*>(lds + 16u * c);
        if (final) {
            if (lane < rem && body + lane >= skip) text[base + body + lane] = lds[body + lane];
            __syncthreads();
            return;
        }
        const char c = lane < rem ? lds[body + lane] : (char)0;
        __syncthreads();
        if (lane < rem) lds[lane] = c;
        base += body;
        if (n_chunks) skip = 0;
        fill = rem;
        __syncthreads();
    }

    // n bytes, byte i = f(i), the wave's lanes side by side
    template <class F>
    SAM_INLINE void emit(uint64_t n64, F f) {
        if (base + fill + n64 > end) over = true, n64 = end - (base + fill);
        const uint32_t lane = threadIdx.x;
        uint64_t done = 0;
        while (done < n64) {
            const uint32_t m = (uint32_t)(n64 - done < (uint64_t)(SAM_BUF - fill) ? n64 - done : (uint64_t)(SAM_BUF - fill));
            for (uint32_t i = lane; i < m; i += 64) lds[fill + i] = f(done + i);
            fill += m, done += m;
            if (fill == SAM_BUF) flush(false);
        }
    }
    SAM_INLINE void put(char c) {
        emit(1, [c](uint64_t) { return c; });
    }
    SAM_INLINE void num(int64_t v) {
        const uint32_t n = num_len(v);
        emit(n, [v, n](uint64_t i) { return num_char(v, n, (uint32_t)i); });
    }
    SAM_INLINE void bytes(const char* s, uint64_t n) {
        emit(n, [s](uint64_t i) { return s[i]; });
    }
    // "\tXX:t:" and the like, up to 8 characters packed in a word, first character lowest
    SAM_INLINE void lit(uint64_t packed, uint32_t n) {
        emit(n, [packed](uint64_t i) { return (char)((packed >> (8 * i)) & 0xff); });
    }
    // a CIGAR: a lane per word, the words' widths summed along the wave
    SAM_INLINE void cigar(const uint32_t* w, int n, int hard) {
        const uint32_t lane = threadIdx.x;
        for (int j0 = 0; j0 < n; j0 += 64) {
            if (SAM_BUF - fill < 64 * 11) flush(false);
            const bool on = j0 + (int)lane < n;
            const uint32_t word = on ? w[j0 + lane] : 0u;
            const uint32_t nd = ndig32(word >> 4), width = on ? nd + 1 : 0u;
            uint32_t incl = width;
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = __shfl_up(incl, d);
                if ((int)lane >= d) incl += up;
            }
            uint32_t total = __shfl(incl, 63);
            if (base + fill + total > end) {  // (never expected) stage nothing rather than part of it
                over = true;
                return;
            }
            if (on) {
                char* p = lds + fill + (incl - width);
                uint32_t x = word >> 4;
                for (int d = (int)nd - 1; d >= 0; --d) p[d] = (char)('0' + x % 10u), x /= 10u;
                p[nd] = cigar_letter(word & 0xf, hard);
            }
            fill += total;
        }
    }
};

// a literal of up to 8 characters as Out::lit takes it
template <size_t N>
constexpr uint64_t pack8(const char (&s)[N]) {
    static_assert(N - 1 <= 8, "at most 8 characters");
    uint64_t v = 0;
    for (size_t i = 0; i + 1 < N; ++i) v |= (uint64_t)(uint8_t)s[i] << (8 * i);
    return v;
}
#define LIT(s) pack8(s), (uint32_t)(sizeof(s) - 1)

// RG:Z (software/bwamem.c:1303); the comment and the newline (:1325-1326)
SAM_INLINE void write_rg(const SamParams& P, Out& o) {
    if (P.rg_len) o.lit(LIT("\tRG:Z:")), o.bytes(P.rg, P.rg_len);
}
SAM_INLINE void write_end(const SamParams& P, Out& o, uint32_t r) {
    const uint32_t cl = comment_len_of(P, r);
    if (cl) o.put('\t'), o.bytes(P.comments + P.comment_off[r], cl);
    o.put('\n');
}

// SEQ and QUAL of the read's [qb, qe) on one strand (software/bwamem.c:1266-1294)
SAM_INLINE void write_seq(const SamParams& P, Out& o, uint32_t r, int qb, int qe, int is_rev) {
    const uint64_t off = P.offs[r];
    const uint8_t* s = P.codes + off;
    const uint64_t n = (uint64_t)(qe - qb);
    if (!is_rev) o.emit(n, [s, qb](uint64_t i) { return base_fwd(s[qb + i]); });
    else o.emit(n, [s, qe](uint64_t i) { return base_rev(s[qe - 1 - i]); });
    o.put('\t');
    if (!P.qual) {
        o.put('*');
        return;
    }
    const char* q = P.qual + off;
    if (!is_rev) o.emit(n, [q, qb](uint64_t i) { return q[qb + i]; });
    else o.emit(n, [q, qe](uint64_t i) { return q[qe - 1 - i]; });
}

// what the lines of one read share in the paired-end text: the mate, extra_flag & 2, and the
// MAPQ that replaces the record's in branch 1 and 2 (-1: none)
struct PeRead {
    const SamPeParams* X;
    Mate M;
    int proper, mapq;
};

// RNEXT, PNEXT and TLEN of a line (software/bwamem.c:1249-1260)
SAM_INLINE void write_mate(const SamParams& P, Out& o, const PeLine& L) {
    if (L.mrid < 0) {
        o.lit(LIT("*\t0\t0"));
        return;
    }
    if (L.eq) o.put('=');
    else o.bytes(P.ctg_names + P.ctg_name_off[L.mrid], ctg_name_len(P, L.mrid));
    o.put('\t'), o.num(L.pnext), o.put('\t'), o.num(L.tlen);
}

// mem_aln2sam of list[which] = record k of read r (software/bwamem.c:1214-1327); PE: with the
// mate C->M, else m == 0
template <bool PE>
SAM_INLINE void write_record(const SamParams& P, Out& o, uint32_t r, uint64_t lo, uint64_t hi, uint64_t k,
                                    bool others, const PeRead* C) {
    const Aln A = P.alns[k];
    RecV V = rec_of(P, k);
    const int rid = P.rid[k], which = (int)(k - lo);
    const int l_seq = (int)(P.offs[r + 1] - P.offs[r]);
    const uint32_t* cg = P.cigar + A.cigar_off;
    PeLine L;
    if (PE) {
        L = pe_line(P, r, C->M, C->proper, V.flag, rid, A, (int)C->X->rlen[k]);           // :1221-1229
        if (C->mapq >= 0) V.mapq = C->mapq;
    }
    const int flag = PE ? L.flag : V.flag | (A.is_rev ? 0x10 : 0);                        // :1228
    o.bytes(P.names + P.name_off[r], name_len_of(P, r)), o.put('\t');                     // :1232
    o.num((flag & 0xffff) | (flag & 0x10000 ? 0x100 : 0)), o.put('\t');                   // :1233
    o.bytes(P.ctg_names + P.ctg_name_off[rid], ctg_name_len(P, rid)), o.put('\t');        // :1235
    o.num(A.pos - P.ctg_off[rid] + 1), o.put('\t');                                       // :1236
    o.num(V.mapq), o.put('\t');                                                           // :1237
    if (A.n_cigar) o.cigar(cg, A.n_cigar, which != 0);                                    // :1238-1243
    else o.put('*');
    if (PE) o.put('\t'), write_mate(P, o, L), o.put('\t');                                // :1246-1261
    else o.lit(LIT("\t*\t0\t0\t"));                                                       // :1246, 1260-1261
    if (flag & 0x100) {                                                                   // :1264-1265
        o.lit(LIT("*\t*"));
    } else {
        int qb, qe;
        seq_range(cg, A.n_cigar, which, A.is_rev, l_seq, &qb, &qe);
        write_seq(P, o, r, qb, qe, A.is_rev);
    }
    if (A.n_cigar) {                                                                      // :1297-1300
        o.lit(LIT("\tNM:i:")), o.num(A.NM);
        o.lit(LIT("\tMD:Z:")), o.bytes(P.md + A.md_off, (uint64_t)A.md_len);
    }
    if (V.score >= 0) o.lit(LIT("\tAS:i:")), o.num(V.score);                              // :1301
    if (V.xs >= 0) o.lit(LIT("\tXS:i:")), o.num(V.xs);                                    // :1302
    write_rg(P, o);                                                                       // :1303
    if (!(flag & 0x100) && others) {                                                      // :1304-1323
        o.lit(LIT("\tSA:Z:"));
        for (uint64_t i = lo; i < hi; ++i) {
            if (i == k || P.sa_len[i] == 0) continue;                                     // :1312
            const Aln B = P.alns[i];
            const RecV W = rec_of(P, i);
            const int rb = P.rid[i];
            o.bytes(P.ctg_names + P.ctg_name_off[rb], ctg_name_len(P, rb)), o.put(',');   // :1313
            o.num(B.pos - P.ctg_off[rb] + 1), o.put(',');                                 // :1314
            o.put(B.is_rev ? '-' : '+'), o.put(',');                                      // :1315
            o.cigar(P.cigar + B.cigar_off, B.n_cigar, 0);                                 // :1316-1318
            o.put(','), o.num(W.mapq);                                                    // :1319
            o.put(','), o.num(B.NM);                                                      // :1320
            o.put(';');                                                                   // :1321
        }
    }
    write_end(P, o, r);                                                                   // :1325-1326
}

__global__ __launch_bounds__(64) void sam_write_kernel(SamParams P) {
    for (uint32_t r = blockIdx.x; r < P.n_reads; r += gridDim.x) {
        const uint64_t t0 = P.text_off[r], t1 = P.text_off[r + 1];
        if (t1 <= t0) continue;  // the host's read
        Out o;
        o.text = P.text, o.base = t0 & ~15ull, o.end = t1, o.fill = o.skip = (uint32_t)(t0 & 15), o.over = false;
        const uint64_t lo = P.rec_off[r], hi = P.rec_off[r + 1];
        if (lo == hi) {  // t = mem_reg2aln(.., 0): software/bwamem.c:1381-1385
            o.bytes(P.names + P.name_off[r], name_len_of(P, r));
            o.lit(LIT("\t4\t*\t0\t0")), o.lit(LIT("\t*\t*\t0\t0")), o.put('\t');         // :1233, 1245-1246, 1260-1261
            write_seq(P, o, r, 0, (int)(P.offs[r + 1] - P.offs[r]), 0);
            o.lit(LIT("\tAS:i:0")), o.lit(LIT("\tXS:i:0"));                               // :1301-1302
            write_rg(P, o);
            write_end(P, o, r);
        } else {
            uint32_t n_prim = 0;
            for (uint64_t k = lo; k < hi; ++k) n_prim += P.sa_len[k] != 0;
            for (uint64_t k = lo; k < hi; ++k) write_record<false>(P, o, r, lo, hi, k, n_prim >= 2, nullptr);
        }
        const bool bad = o.over || o.base + o.fill != t1;
        o.flush(true);
        if (bad && threadIdx.x == 0) atomicAdd(P.cnt + SAM_N_BADLEN, 1u);
    }
}

// the paired-end text, one wave per read: every line against the read's mate
__global__ __launch_bounds__(64) void sam_write_pe_kernel(SamPeParams X) {
    const SamParams& P = X.s;
    for (uint32_t r = blockIdx.x; r < P.n_reads; r += gridDim.x) {
        const uint64_t t0 = P.text_off[r], t1 = P.text_off[r + 1];
        if (t1 <= t0) continue;  // the host's pair
        Out o;
        o.text = P.text, o.base = t0 & ~15ull, o.end = t1, o.fill = o.skip = (uint32_t)(t0 & 15), o.over = false;
        const uint64_t lo = P.rec_off[r], hi = P.rec_off[r + 1];
        PeRead C;
        C.X = &X, C.M = mate_of(X, r);
        if (lo == hi) {  // t = mem_reg2aln(.., 0) against the mate: software/bwamem.c:1381-1385, 1224-1225
            const PeLine L = pe_line_unmapped(P, r, C.M);
            o.bytes(P.names + P.name_off[r], name_len_of(P, r)), o.put('\t');
            o.num(L.flag), o.put('\t');
            if (C.M.has) {                                                                // :1235-1237, 1244
                o.bytes(P.ctg_names + P.ctg_name_off[L.mrid], ctg_name_len(P, L.mrid)), o.put('\t');
                o.num(L.pnext), o.lit(LIT("\t0\t*\t"));
            } else {
                o.lit(LIT("*\t0\t0\t*\t"));                                               // :1245
            }
            write_mate(P, o, L), o.put('\t');
            write_seq(P, o, r, 0, (int)(P.offs[r + 1] - P.offs[r]), C.M.has && C.M.is_rev);
            o.lit(LIT("\tAS:i:0")), o.lit(LIT("\tXS:i:0"));                               // :1301-1302
            write_rg(P, o);
            write_end(P, o, r);
        } else {
            const SamPair S = X.pairs[r >> 1];
            C.proper = proper_of(X, r, C.M), C.mapq = S.mode <= 0 ? -1 : (r & 1u) ? S.mapq[1] : S.mapq[0];
            uint32_t n_prim = 0;
            for (uint64_t k = lo; k < hi; ++k) n_prim += P.sa_len[k] != 0;
            for (uint64_t k = lo; k < hi; ++k) write_record<true>(P, o, r, lo, hi, k, n_prim >= 2, &C);
        }
        const bool bad = o.over || o.base + o.fill != t1;
        o.flush(true);
        if (bad && threadIdx.x == 0) atomicAdd(P.cnt + SAM_N_BADLEN, 1u);
    }
}

}  // namespace
}  // namespace smem

extern "C" hipError_t smem_launch_sam_len(const smem::SamParams* P, hipStream_t st) {
    if (P->n_rec)
        hipLaunchKernelGGL(smem::sam_len_kernel, dim3((unsigned)((P->n_rec + 255) / 256)), dim3(256), 0, st, *P);
    if (P->n_reads)
        hipLaunchKernelGGL(smem::sam_read_kernel, dim3((unsigned)((P->n_reads + 255) / 256)), dim3(256), 0, st, *P);
    return hipGetLastError();
}

extern "C" hipError_t smem_launch_sam_pe_len(const smem::SamPeParams* X, hipStream_t st) {
    const smem::SamParams& P = X->s;
    if (P.n_rec)
        hipLaunchKernelGGL(smem::sam_len_pe_kernel, dim3((unsigned)((P.n_rec + 255) / 256)), dim3(256), 0, st, *X);
    if (P.n_reads)
        hipLaunchKernelGGL(smem::sam_read_pe_kernel, dim3((unsigned)((P.n_reads + 255) / 256)), dim3(256), 0, st, *X);
    return hipGetLastError();
}

extern "C" hipError_t smem_launch_sam_write(const smem::SamParams* P, hipStream_t st) {
    if (P->n_reads == 0) return hipSuccess;
    const unsigned grid = P->n_reads < (uint32_t)smem::SAM_WRITE_BLOCKS_MAX ? P->n_reads : (unsigned)smem::SAM_WRITE_BLOCKS_MAX;
    hipLaunchKernelGGL(smem::sam_write_kernel, dim3(grid), dim3(64), 0, st, *P);
    return hipGetLastError();
}

extern "C" hipError_t smem_launch_sam_pe_write(const smem::SamPeParams* X, hipStream_t st) {
    const uint32_t n = X->s.n_reads;
    if (n == 0) return hipSuccess;
    const unsigned grid = n < (uint32_t)smem::SAM_WRITE_BLOCKS_MAX ? n : (unsigned)smem::SAM_WRITE_BLOCKS_MAX;
    hipLaunchKernelGGL(smem::sam_write_pe_kernel, dim3(grid), dim3(64), 0, st, *X);
    return hipGetLastError();
}

// this file's code object loaded on the current device (see smem_preload_seed)
extern "C" hipError_t smem_preload_sam(void) {
    hipFuncAttributes a;
    hipError_t e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(smem::sam_len_kernel));
    if (e == hipSuccess) e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(smem::sam_read_kernel));
    if (e == hipSuccess) e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(smem::sam_write_kernel));
    if (e == hipSuccess) e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(smem::sam_len_pe_kernel));
    if (e == hipSuccess) e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(smem::sam_read_pe_kernel));
    if (e == hipSuccess) e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(smem::sam_write_pe_kernel));
    return e;
}
