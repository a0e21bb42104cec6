// Long reads of an aligned BAM: which mapped records span a VNTR window, and the piece of each that covers it
// (VNTRFinder.check_if_pacbio_mapped_read_spans_vntr, vntr_finder.py:373-420, restated from SAMv1 section 1.4.6).
//
// Aligned bases are those of M, = and X ops; S and I consume the query only, D and N the reference only, H and P neither
// (pysam's get_reference_positions; with full_length the query index counts S and I as well, so it indexes SEQ as stored).
// For the window [vs, ve), F flank bases and MIN the minimum flank:
//   spanning   first aligned reference position <= vs - MIN and last aligned > ve + MIN
//   counts     aligned bases with reference position in [vs - F, vs) -> left, [vs, ve) -> tr, [ve, ve + F) -> right;
//              rs = query index of the first aligned base in the left range, re = that of the first in the right range
//   rejected   left < MIN or right < MIN
//   piece      SEQ[rs : re + right], clamped to l_seq as a Python slice (an insertion in the right flank shortens it, a
//              deletion lengthens it, as in the reference; mapped reads are on the reference strand already)
// The per-op intersection and the final rule are host + device code: the host twin walks the CIGAR op by op, the span
// kernel one op per lane with a wave-wide scan of the op lengths; both fold the same SpanAcc.
#pragma once
#include <stdint.h>

#include "bam_records.h"

namespace bam {

enum SpanStatus : int32_t {
    SPAN_OK = 0,              // spanning: the piece is SEQ[rs, end)
    SPAN_UNMAPPED = 1,        // flag 0x4
    SPAN_NO_ALIGNED = 2,      // no M / = / X base
    SPAN_NOT_SPANNING = 3,    // first / last aligned position fails the spanning test
    SPAN_SHORT_FLANK = 4,     // left or right flank count below MIN
    SPAN_NO_SEQ = 5,          // l_seq == 0 (pysam: read.seq is None)
    SPAN_CG_TAG = 6,          // CIGAR is the <l_seq>S<ref_len>N placeholder of a CG:B,I tag (not decoded): an error
    SPAN_N_STATUS = 7
};

const int64_t SPAN_NONE = INT64_MAX;

// what the ops fold into: min / max / sums, so any grouping of the ops gives the same result
struct SpanAcc {
    int64_t first_ref, last_ref;        // aligned reference positions (SPAN_NONE / -1 when none)
    int64_t left, tr, right;            // aligned bases in [vs-F, vs), [vs, ve), [ve, ve+F)
    int64_t rs, re;                     // query index of the first aligned base of the left / right range (SPAN_NONE)
};

BGZF_HD inline void span_init(SpanAcc &a)
{
    a.first_ref = SPAN_NONE;
    a.last_ref = -1;
    a.left = a.tr = a.right = 0;
    a.rs = a.re = SPAN_NONE;
}

BGZF_HD inline int64_t span_min(int64_t a, int64_t b) { return a < b ? a : b; }
BGZF_HD inline int64_t span_max(int64_t a, int64_t b) { return a > b ? a : b; }

BGZF_HD inline void span_merge(SpanAcc &a, const SpanAcc &b)
{
    a.first_ref = span_min(a.first_ref, b.first_ref);
    a.last_ref = span_max(a.last_ref, b.last_ref);
    a.left += b.left;
    a.tr += b.tr;
    a.right += b.right;
    a.rs = span_min(a.rs, b.rs);
    a.re = span_min(a.re, b.re);
}

BGZF_HD inline bool op_aligned(uint32_t op) { return op == 0 || op == 7 || op == 8; }                 // M = X
BGZF_HD inline bool op_query(uint32_t op) { return op == 0 || op == 1 || op == 4 || op == 7 || op == 8; }   // M I S = X
BGZF_HD inline bool op_ref(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }     // M D N = X

// bases [a, b) of an aligned op covering reference [r0, r0 + len) from query index q0: count, and the query index of the first
BGZF_HD inline int64_t span_range(int64_t q0, int64_t r0, int64_t len, int64_t a, int64_t b, int64_t *first_q)
{
    const int64_t lo = span_max(r0, a), hi = span_min(r0 + len, b);
    if (hi <= lo) return 0;
    *first_q = q0 + (lo - r0);
    return hi - lo;
}

// fold one op (query index q0 and reference position r0 where it starts) into `acc`
BGZF_HD inline void span_op(SpanAcc &acc, uint32_t op, int64_t len, int64_t q0, int64_t r0, int64_t vs, int64_t ve, int64_t F)
{
    if (!op_aligned(op) || len <= 0) return;
    acc.first_ref = span_min(acc.first_ref, r0);
    acc.last_ref = span_max(acc.last_ref, r0 + len - 1);
    int64_t q = SPAN_NONE;
    const int64_t nl = span_range(q0, r0, len, vs - F, vs, &q);
    if (nl) { acc.left += nl; acc.rs = span_min(acc.rs, q); }
    int64_t qt = 0;
    acc.tr += span_range(q0, r0, len, vs, ve, &qt);
    const int64_t nr = span_range(q0, r0, len, ve, ve + F, &q);
    if (nr) { acc.right += nr; acc.re = span_min(acc.re, q); }
}

// the CG:B,I placeholder: exactly two ops, <l_seq>S then <ref_len>N (SAMv1 1.4.6 / htslib)
BGZF_HD inline bool cigar_is_cg_placeholder(const uint8_t *buf, const Record &r)
{
    if (r.n_cigar != 2 || r.l_seq <= 0) return false;
    const uint32_t c0 = rd_u32(buf + r.cigar_at), c1 = rd_u32(buf + r.cigar_at + 4);
    return (c0 & 15) == 4 && (int64_t)(c0 >> 4) == (int64_t)r.l_seq && (c1 & 15) == 3;
}

struct Span {
    int32_t status;
    int64_t rs, end, left, tr, right;
};

// the rule over the folded ops
BGZF_HD inline Span span_finish(const SpanAcc &a, const Record &r, int64_t vs, int64_t ve, int64_t MIN)
{
    Span s;
    s.rs = s.end = 0;
    s.left = a.left;
    s.tr = a.tr;
    s.right = a.right;
    if (a.last_ref < 0) s.status = SPAN_NO_ALIGNED;
    else if (!(a.first_ref <= vs - MIN && ve + MIN < a.last_ref)) s.status = SPAN_NOT_SPANNING;
    else if (a.left < MIN || a.right < MIN) s.status = SPAN_SHORT_FLANK;
    else if (r.l_seq == 0) s.status = SPAN_NO_SEQ;
    else {
        s.status = SPAN_OK;
        const int64_t n = r.l_seq;
        s.rs = span_min(a.rs, n);
        s.end = span_max(s.rs, span_min(a.re + a.right, n));
    }
    return s;
}

// status before the CIGAR is walked (SPAN_OK = walk it)
BGZF_HD inline int32_t span_precheck(const uint8_t *buf, const Record &r)
{
    if (r.flag & 4) return SPAN_UNMAPPED;
    if (cigar_is_cg_placeholder(buf, r)) return SPAN_CG_TAG;
    return SPAN_OK;
}

// the host twin: the CIGAR op by op
inline Span span_host(const uint8_t *buf, const Record &r, int64_t vs, int64_t ve, int64_t F, int64_t MIN)
{
    Span s = {span_precheck(buf, r), 0, 0, 0, 0, 0};
    if (s.status != SPAN_OK) return s;
    SpanAcc acc;
    span_init(acc);
    int64_t q = 0, ref = r.pos;
    for (int32_t i = 0; i < r.n_cigar; ++i) {
        const uint32_t c = rd_u32(buf + r.cigar_at + 4 * (int64_t)i), op = c & 15;
        const int64_t len = c >> 4;
        span_op(acc, op, len, q, ref, vs, ve, F);
        if (op_query(op)) q += len;
        if (op_ref(op)) ref += len;
    }
    return span_finish(acc, r, vs, ve, MIN);
}

// text of a spanning pair: name | SEQ[rs, end)
BGZF_HD inline void decode_piece_base(const uint8_t *buf, const Record &r, int64_t i, uint8_t *dst)
{
    const char *codes = "=ACMGRSVTWYHKDBN";
    const uint8_t b = buf[r.seq_at + i / 2];
    *dst = (uint8_t)codes[(i & 1) ? (b & 15) : (b >> 4)];
}

// pairs of a mapped record with the windows it overlaps (SamFile.fetch's test of in_windows): windows of a reference sorted
// by start, win_end[k] their own ends, win_maxend the running maximum.  Scans back from the last window starting before the
// record's end while the running maximum still reaches past its start; calls emit(k) for every overlapping k, in descending k.
template <class Emit>
BGZF_HD inline int32_t window_pairs(const Record &r, int64_t ref_end, int32_t n_ref, const int32_t *win_ptr, const int64_t *win_start,
                                    const int64_t *win_end, const int64_t *win_maxend, Emit emit)
{
    if ((r.flag & 4) || r.ref < 0 || r.ref >= n_ref) return 0;
    const int64_t s = r.pos, e = ref_end >= 0 ? ref_end : (int64_t)r.pos + 1;
    int32_t lo = win_ptr[r.ref], hi = win_ptr[r.ref + 1];
    const int32_t first = lo;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (win_start[mid] < e) lo = mid + 1;
        else hi = mid;
    }
    int32_t n = 0;
    for (int32_t k = lo - 1; k >= first && win_maxend[k] > s; --k)
        if (win_end[k] > s) { emit(k); ++n; }
    return n;
}

}  // namespace bam

#if defined(__HIPCC__)
namespace bam {

const int SPAN_OUT = 8;     // per pair: status, rs, end, left, tr, right, name length, whole-decode text bytes

// one thread per record: unmapped records are kept whole (as select_kernel keeps them); a mapped record's (record, window)
// pairs go to pair_rec / pair_win (slot by atomic; the host orders them); n_counters = {kept, pairs, bad record, whole bytes}
__global__ void span_select_kernel(const uint8_t *buf, const int64_t *offs, int64_t n_rec, int32_t n_ref, const int32_t *win_ptr,
                                   const int64_t *win_start, const int64_t *win_end, const int64_t *win_maxend,
                                   unsigned long long *counters, int64_t *kept_idx, int64_t *kept_bytes, int64_t kept_cap,
                                   int64_t *pair_rec, int32_t *pair_win, int64_t pair_cap)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec) return;
    Record r;
    if (!parse(buf, offs[i], r)) {
        atomicMin(counters + 2, (unsigned long long)i);
        return;
    }
    if (r.flag & 4) {
        const unsigned long long slot = atomicAdd(counters, 1ull);
        if ((int64_t)slot < kept_cap) {
            kept_idx[slot] = i;
            kept_bytes[slot] = text_bytes(buf, r);
        }
        return;
    }
    const int64_t end = reference_end(buf, r);
    const int32_t n = window_pairs(r, end, n_ref, win_ptr, win_start, win_end, win_maxend, [&](int32_t k) {
        const unsigned long long slot = atomicAdd(counters + 1, 1ull);
        if ((int64_t)slot < pair_cap) {
            pair_rec[slot] = i;
            pair_win[slot] = k;
        }
    });
    if (n) atomicAdd(counters + 3, (unsigned long long)text_bytes(buf, r));     // what the whole decode would have produced
}

template <class T> __device__ __forceinline__ T wave_sum(T v)
{
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
template <class T> __device__ __forceinline__ T wave_min(T v)
{
    for (int d = 32; d >= 1; d >>= 1) v = span_min(v, __shfl_xor(v, d, 64));
    return v;
}
template <class T> __device__ __forceinline__ T wave_max(T v)
{
    for (int d = 32; d >= 1; d >>= 1) v = span_max(v, __shfl_xor(v, d, 64));
    return v;
}

// one wavefront per pair: the CIGAR 64 ops at a time, one op per lane; an inclusive scan of the query and reference lengths
// across the wave (carried from chunk to chunk) gives each op where it starts; each lane folds its ops, the wave reduces.
// win_start / win_end are the sorted windows; out[SPAN_OUT] per pair.
__global__ void __launch_bounds__(256) span_kernel(const uint8_t *buf, const int64_t *offs, const int64_t *pair_rec,
                                                   const int32_t *pair_win, int64_t n_pairs, const int64_t *win_start,
                                                   const int64_t *win_end, int64_t F, int64_t MIN, int64_t *out)
{
    const int64_t p = (int64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (p >= n_pairs) return;
    Record r;
    parse(buf, offs[pair_rec[p]], r);            // the select kernel checked it
    const int64_t vs = win_start[pair_win[p]], ve = win_end[pair_win[p]];
    Span s = {span_precheck(buf, r), 0, 0, 0, 0, 0};
    if (s.status == SPAN_OK) {
        SpanAcc acc;
        span_init(acc);
        int64_t q_base = 0, r_base = r.pos;
        for (int32_t c0 = 0; c0 < r.n_cigar; c0 += 64) {
            const int32_t i = c0 + lane;
            uint32_t op = 9;                      // past the end: consumes nothing
            int64_t len = 0;
            if (i < r.n_cigar) {
                const uint32_t c = rd_u32(buf + r.cigar_at + 4 * (int64_t)i);
                op = c & 15;
                len = c >> 4;
            }
            const int64_t ql = op_query(op) ? len : 0, rl = op_ref(op) ? len : 0;
            int64_t qs = ql, rsum = rl;           // inclusive scans
            for (int d = 1; d < 64; d <<= 1) {
                const int64_t qa = __shfl_up(qs, d, 64), ra = __shfl_up(rsum, d, 64);
                if (lane >= d) { qs += qa; rsum += ra; }
            }
            span_op(acc, op, len, q_base + qs - ql, r_base + rsum - rl, vs, ve, F);
            q_base += __shfl(qs, 63, 64);
            r_base += __shfl(rsum, 63, 64);
        }
        acc.first_ref = wave_min(acc.first_ref);
        acc.last_ref = wave_max(acc.last_ref);
        acc.left = wave_sum(acc.left);
        acc.tr = wave_sum(acc.tr);
        acc.right = wave_sum(acc.right);
        acc.rs = wave_min(acc.rs);
        acc.re = wave_min(acc.re);
        s = span_finish(acc, r, vs, ve, MIN);
    }
    if (lane == 0) {
        int64_t *o = out + SPAN_OUT * p;
        o[0] = s.status;
        o[1] = s.rs;
        o[2] = s.end;
        o[3] = s.left;
        o[4] = s.tr;
        o[5] = s.right;
        o[6] = r.l_name - 1;
        o[7] = 0;
    }
}

// one wavefront per spanning pair: name | SEQ[rs, end), 4-bit codes unpacked, at text + text_off[k]
__global__ void __launch_bounds__(256) trim_decode_kernel(const uint8_t *buf, const int64_t *offs, const int64_t *rec,
                                                          const int64_t *rs, const int64_t *end, const int64_t *text_off,
                                                          int64_t n, uint8_t *text)
{
    const int64_t k = (int64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (k >= n) return;
    Record r;
    parse(buf, offs[rec[k]], r);
    uint8_t *dst = text + text_off[k];
    const int64_t nl = r.l_name - 1;
    for (int64_t i = lane; i < nl; i += 64) dst[i] = buf[r.name_at + i];
    dst += nl;
    const int64_t a = rs[k], len = end[k] - a;
    for (int64_t i = lane; i < len; i += 64) decode_piece_base(buf, r, a + i, dst + i);
}

}  // namespace bam
#endif
