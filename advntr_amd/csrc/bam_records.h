// BAM records (SAMv1 section 4.2) in inflated BGZF output: the record-chain walk, the selection of the records the Illumina
// path reads, and their decode into text.  The cores are host + device code (BGZF_HD): the kernels run them one thread per
// block (walk) or per record (select, decode); the host runs the same code for the sequential fallback walk and for
// advntr_bam_walk_host / advntr_bam_decode_host.
//
// Record layout: int32 block_size, then refID i32 | pos i32 | l_read_name u8 | mapq u8 | bin u16 | n_cigar_op u16 | flag u16 |
// l_seq i32 | next_refID i32 | next_pos i32 | tlen i32 | read_name[l_read_name] (NUL-terminated) | cigar u32[n_cigar_op] |
// seq u8[(l_seq+1)/2] | qual u8[l_seq] | tags.  Every field read here is bounded by the record's block_size and the buffer.
#pragma once
#include <stdint.h>

#include "bgzf_inflate.h"

namespace bam {

const int32_t MIN_RECORD = 32;      // the fixed part after block_size

BGZF_HD inline uint32_t rd_u32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
BGZF_HD inline int32_t rd_i32(const uint8_t *p) { return (int32_t)rd_u32(p); }
BGZF_HD inline uint32_t rd_u16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }

// Walk the record chain from `p` (assumed to be a record start) over every record that starts before `stop`.  Returns the
// first position at or past `stop` where a record starts, or the start of the first record that does not fit in buf[0, n)
// (the carry into the next chunk).  *count = complete records walked; offs (optional) receives their offsets.  *bad = 1 when
// a block_size below the fixed part was met (the assumed start was wrong, or the file is malformed).
BGZF_HD inline int64_t walk(const uint8_t *buf, int64_t n, int64_t p, int64_t stop, int64_t *offs, int64_t cap, int64_t *count,
                            int *bad)
{
    int64_t c = 0;
    *bad = 0;
    while (p < stop) {
        if (p + 4 > n) break;
        const int32_t bs = rd_i32(buf + p);
        if (bs < MIN_RECORD) { *bad = 1; break; }
        if (p + 4 + (int64_t)bs > n) break;
        if (offs && c < cap) offs[c] = p;
        ++c;
        p += 4 + (int64_t)bs;
    }
    *count = c;
    return p;
}

struct Record {
    int32_t ref, pos, flag, mapq, n_cigar, l_seq, l_name;
    int64_t cigar_at, seq_at, qual_at, name_at;
};

// Fields of the record at `off` (its block_size fits in the buffer: walk() checked).  False when the variable-length parts
// overrun the record.
BGZF_HD inline bool parse(const uint8_t *buf, int64_t off, Record &r)
{
    const uint8_t *p = buf + off;
    const int64_t bs = rd_i32(p);
    r.ref = rd_i32(p + 4);
    r.pos = rd_i32(p + 8);
    r.l_name = p[12];
    r.mapq = p[13];
    r.n_cigar = (int32_t)rd_u16(p + 16);
    r.flag = (int32_t)rd_u16(p + 18);
    r.l_seq = rd_i32(p + 20);
    if (r.l_seq < 0 || r.l_name < 1) return false;
    r.name_at = off + 36;
    r.cigar_at = r.name_at + r.l_name;
    r.seq_at = r.cigar_at + 4 * (int64_t)r.n_cigar;
    r.qual_at = r.seq_at + ((int64_t)r.l_seq + 1) / 2;
    return r.qual_at + r.l_seq <= off + 4 + bs;
}

// one past the last aligned reference base (M D N = X), -1 for an unmapped record or a record without CIGAR (pysam: None)
BGZF_HD inline int64_t reference_end(const uint8_t *buf, const Record &r)
{
    if ((r.flag & 4) || r.n_cigar == 0) return -1;
    int64_t span = 0;
    for (int32_t i = 0; i < r.n_cigar; ++i) {
        const uint32_t c = rd_u32(buf + r.cigar_at + 4 * (int64_t)i), op = c & 15;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += c >> 4;
    }
    return (int64_t)r.pos + span;
}

// SamFile.fetch's test for one window list: a mapped record on `ref` whose [pos, end) overlaps a window [s, e) half-open, end
// = reference_end or pos + 1 without CIGAR.  Windows of a reference are sorted by start; win_maxend[k] = max end of the first
// k + 1 of them.
BGZF_HD inline bool in_windows(const Record &r, int64_t ref_end, int32_t n_ref, const int32_t *win_ptr, const int64_t *win_start,
                               const int64_t *win_maxend)
{
    if ((r.flag & 4) || r.ref < 0 || r.ref >= n_ref) return false;
    const int64_t s = r.pos, e = ref_end >= 0 ? ref_end : (int64_t)r.pos + 1;
    int32_t lo = win_ptr[r.ref], hi = win_ptr[r.ref + 1];
    const int32_t first = lo;
    while (lo < hi) {                       // windows starting before e: [first, lo)
        const int32_t mid = lo + (hi - lo) / 2;
        if (win_start[mid] < e) lo = mid + 1;
        else hi = mid;
    }
    return lo > first && win_maxend[lo - 1] > s;
}

BGZF_HD inline int digits(uint32_t v)
{
    int d = 1;
    while (v >= 10) { v /= 10; ++d; }
    return d;
}

// text bytes of a kept record: name, sequence ('*' when l_seq is 0), qualities (raw, only when present), CIGAR ('*' when none)
BGZF_HD inline int64_t text_bytes(const uint8_t *buf, const Record &r)
{
    int64_t cig = r.n_cigar ? 0 : 1;
    for (int32_t i = 0; i < r.n_cigar; ++i) cig += digits(rd_u32(buf + r.cigar_at + 4 * (int64_t)i) >> 4) + 1;
    const bool qual = r.l_seq > 0 && buf[r.qual_at] != 0xff;
    return (r.l_name - 1) + (r.l_seq ? r.l_seq : 1) + (qual ? r.l_seq : 0) + cig;
}

const int FIELDS = 10;      // per decoded record: ref, pos, flag, mapq, ref_end (-1 = None), name_len, seq_len, qual_len, cigar_len, 0

// Decode the record at `off` into fields[FIELDS] and text (text_bytes(...) of room): name | seq | qual | cigar
BGZF_HD inline void decode(const uint8_t *buf, const Record &r, int32_t *fields, uint8_t *text)
{
    const char *codes = "=ACMGRSVTWYHKDBN", *ops = "MIDNSHP=X???????";
    int64_t t = 0;
    for (int32_t i = 0; i < r.l_name - 1; ++i) text[t++] = buf[r.name_at + i];
    if (r.l_seq == 0) text[t++] = '*';
    for (int32_t i = 0; i < r.l_seq; ++i) {
        const uint8_t b = buf[r.seq_at + i / 2];
        text[t++] = (uint8_t)codes[(i & 1) ? (b & 15) : (b >> 4)];
    }
    const bool qual = r.l_seq > 0 && buf[r.qual_at] != 0xff;
    if (qual)
        for (int32_t i = 0; i < r.l_seq; ++i) text[t++] = buf[r.qual_at + i];
    const int64_t cig0 = t;
    if (r.n_cigar == 0) text[t++] = '*';
    for (int32_t i = 0; i < r.n_cigar; ++i) {
        const uint32_t c = rd_u32(buf + r.cigar_at + 4 * (int64_t)i), len = c >> 4;
        const int d = digits(len);
        uint32_t v = len;
        for (int k = d - 1; k >= 0; --k) { text[t + k] = (uint8_t)('0' + v % 10); v /= 10; }
        t += d;
        text[t++] = (uint8_t)ops[c & 15];
    }
    const int64_t end = reference_end(buf, r);
    fields[0] = r.ref;
    fields[1] = r.pos;
    fields[2] = r.flag;
    fields[3] = r.mapq;
    fields[4] = (int32_t)end;
    fields[5] = r.l_name - 1;
    fields[6] = r.l_seq ? r.l_seq : 1;
    fields[7] = qual ? r.l_seq : 0;
    fields[8] = (int32_t)(t - cig0);
    fields[9] = 0;
}

}  // namespace bam

#if defined(__HIPCC__)
namespace bam {

// one thread per block: the chain walk from the block's assumed first record start[b] over the records starting before the
// block's end; end_out[b] = where the walk stopped (-1 when it met an impossible block_size), count_out[b] = records.  With
// offs != nullptr (second pass, starts verified) the offsets go to offs[base[b] ...].
__global__ void walk_blocks_kernel(const uint8_t *buf, int64_t n, const int64_t *start, const int64_t *stop, int32_t n_blocks,
                                   int64_t *end_out, int32_t *count_out, const int64_t *base, int64_t *offs)
{
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= n_blocks) return;
    int64_t count = 0;
    int bad = 0;
    const int64_t cap = offs ? (int64_t)count_out[b] : 0;
    const int64_t e = walk(buf, n, start[b], stop[b], offs ? offs + base[b] : nullptr, cap, &count, &bad);
    if (!offs) {
        end_out[b] = bad ? -1 : e;
        count_out[b] = (int32_t)count;
    }
}

// one thread per record: keep (a) the first `head_left` records of the file, (b) mapped records that overlap a window,
// (c) unmapped records; slot by atomic, kept_idx / kept_bytes unordered (the host sorts the few kept records).  A record whose
// variable-length parts overrun it sets *bad_first to its index (smallest wins).
__global__ void select_kernel(const uint8_t *buf, const int64_t *offs, int64_t n_rec, int64_t head_left, int32_t n_ref,
                              const int32_t *win_ptr, const int64_t *win_start, const int64_t *win_maxend,
                              unsigned long long *n_kept, int64_t *kept_idx, int64_t *kept_bytes, int64_t kept_cap,
                              unsigned long long *bad_first)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec) return;
    Record r;
    if (!parse(buf, offs[i], r)) {
        atomicMin(bad_first, (unsigned long long)i);
        return;
    }
    const int64_t end = reference_end(buf, r);
    if (i < head_left || (r.flag & 4) || in_windows(r, end, n_ref, win_ptr, win_start, win_maxend)) {
        const unsigned long long slot = atomicAdd(n_kept, 1ull);
        if ((int64_t)slot < kept_cap) {
            kept_idx[slot] = i;
            kept_bytes[slot] = text_bytes(buf, r);
        }
    }
}

// one thread per kept record (in file order): fields and text
__global__ void decode_kernel(const uint8_t *buf, const int64_t *offs, const int64_t *kept_idx, const int64_t *text_off,
                              int64_t n_kept, int32_t *fields, uint8_t *text)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_kept) return;
    Record r;
    parse(buf, offs[kept_idx[k]], r);
    decode(buf, r, fields + FIELDS * k, text + text_off[k]);
}

}  // namespace bam
#endif
