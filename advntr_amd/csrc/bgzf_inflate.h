// BGZF inflate: RFC 1951 DEFLATE decoding of BGZF blocks, one wavefront per block on the device, and the same decoder core
// on the host (header parsing, and tests/native/asan_inflate.cpp, which compiles this file with g++ under ASan/UBSan).
//
// The decode of the bitstream is wave-uniform: every lane of the wave runs the same decoder over the same bits, so the wave is
// one instruction stream without divergence.  Work that splits over lanes: filling the Huffman lookup tables (one lane per
// coded symbol), stored-block copies, match copies (pieces of min(distance, lanes) bytes: every byte of a piece has its source
// before the piece) and the CRC32 of the output (one stripe per lane, merged with crc32_combine's GF(2) shifts).
// Back-references are read from the block's own output in global memory; a barrier (workgroup-scope release + acquire; the
// workgroup is the one wave) separates the stores of a piece from the loads of the next.
//
// Malformed input never leads to an out-of-bounds access: every bit read is bounded by the block's compressed span, every
// write by the output capacity (ISIZE), and over-subscribed or incomplete code-length sets, invalid symbols and distances
// beyond the output produced so far are block errors.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BGZF_HD __host__ __device__
#else
#define BGZF_HD
#endif

namespace bgzf {

enum Status : int32_t {
    INF_OK = 0,
    INF_BAD_BLOCK_TYPE = 1,     // BTYPE 3
    INF_STORED_LEN = 2,         // stored block: LEN != ~NLEN
    INF_TRUNCATED = 3,          // the bitstream ends before the final block does
    INF_BAD_LENGTHS = 4,        // over-subscribed / incomplete code lengths, repeat overflow, no end-of-block code
    INF_BAD_SYMBOL = 5,         // a code that is not in the table, length symbol 286/287, distance symbol 30/31
    INF_DISTANCE = 6,           // distance beyond the output produced so far
    INF_OVERFLOW = 7,           // more output than ISIZE
    INF_ISIZE = 8,              // less output than ISIZE
    INF_CRC = 9,                // CRC32 of the output differs from the footer's
};

const int MAXBITS = 15, FAST = 9, NLIT = 288, NDIST = 32;

struct Huff {
    uint16_t count[MAXBITS + 1];
    uint16_t offs[MAXBITS + 1];     // index in `sorted` of the first symbol of each length
    uint16_t fast[1 << FAST];       // (symbol << 4) | length for codes up to FAST bits (bit-reversed index); 0 = not there
    uint16_t sorted[NLIT];
};

struct Tables {                     // per wave: 4.6 KiB of LDS on the device
    Huff lit, dist;
    uint8_t lens[NLIT + NDIST];
    uint32_t crc[256];
};

// a "wave" of the host: one lane, no barrier
struct HostWave {
    BGZF_HD int lane() const { return 0; }
    BGZF_HD int lanes() const { return 1; }
    BGZF_HD void sync() const {}
};

BGZF_HD inline uint32_t crc_table_entry(uint32_t n)
{
    uint32_t c = n;
    for (int k = 0; k < 8; ++k) c = c & 1 ? 0xedb88320u ^ (c >> 1) : c >> 1;
    return c;
}

// GF(2) polynomial product modulo the CRC-32 polynomial (zlib's multmodp); `a` is never 0 here (a power of x)
BGZF_HD inline uint32_t multmodp(uint32_t a, uint32_t b)
{
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = b & 1 ? (b >> 1) ^ 0xedb88320u : b >> 1;
    }
    return p;
}

// x^(8 n) modulo the polynomial: the operator that shifts a CRC over n zero bytes
BGZF_HD inline uint32_t x8nmodp(uint32_t n)
{
    uint32_t p = 1u << 31, x2k = 1u << 30;      // x^0, x^1
    for (int k = 0; k < 3; ++k) x2k = multmodp(x2k, x2k);     // x^8
    while (n) {
        if (n & 1) p = multmodp(x2k, p);
        n >>= 1;
        if (n) x2k = multmodp(x2k, x2k);
    }
    return p;
}

// crc32(A || B) from crc32(A), crc32(B) and len(B)
BGZF_HD inline uint32_t crc32_combine(uint32_t crc_a, uint32_t crc_b, uint32_t len_b)
{
    return multmodp(x8nmodp(len_b), crc_a) ^ crc_b;
}

BGZF_HD inline uint32_t crc32_bytes(const uint32_t *table, const uint8_t *p, uint32_t n)
{
    uint32_t c = 0xffffffffu;
    for (uint32_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 0xff] ^ (c >> 8);
    return c ^ 0xffffffffu;
}

template <class W> BGZF_HD inline void fill_crc_table(Tables &T, const W &w)
{
    for (int i = w.lane(); i < 256; i += w.lanes()) T.crc[i] = crc_table_entry((uint32_t)i);
    w.sync();
}

// CRC32 of out[0, n): one stripe per lane, merged in lane order.  Every lane returns the result.
template <class W> BGZF_HD inline uint32_t crc32_wave(Tables &T, const uint8_t *out, uint32_t n, const W &w, uint32_t *scratch)
{
    const uint32_t L = (uint32_t)w.lanes(), stripe = (n + L - 1) / L;
    const uint32_t lo = stripe * (uint32_t)w.lane() < n ? stripe * (uint32_t)w.lane() : n;
    const uint32_t hi = lo + stripe < n ? lo + stripe : n;
    const uint32_t mine = crc32_bytes(T.crc, out + lo, hi - lo);
    if (L == 1) return mine;
    scratch[w.lane()] = mine;
    w.sync();
    uint32_t crc = 0;
    if (w.lane() == 0) {
        const uint32_t shift_full = x8nmodp(stripe);
        for (uint32_t l = 0; l < L; ++l) {
            const uint32_t a = stripe * l < n ? stripe * l : n, b = a + stripe < n ? a + stripe : n;
            if (b == a) break;
            crc = multmodp(b - a == stripe ? shift_full : x8nmodp(b - a), crc) ^ scratch[l];
        }
        scratch[L] = crc;
    }
    w.sync();
    crc = scratch[L];
    w.sync();
    return crc;
}

struct Bits {
    const uint8_t *in;
    uint32_t len, pos;      // next byte to load
    uint64_t buf;
    int cnt;

    BGZF_HD void refill()
    {
        if (cnt <= 32 && pos + 4 <= len) {      // four independent byte loads
            const uint64_t w = (uint64_t)in[pos] | (uint64_t)in[pos + 1] << 8 | (uint64_t)in[pos + 2] << 16 |
                               (uint64_t)in[pos + 3] << 24;
            buf |= w << cnt;
            cnt += 32;
            pos += 4;
        }
        while (cnt <= 56 && pos < len) {
            buf |= (uint64_t)in[pos++] << cnt;
            cnt += 8;
        }
    }
    // n <= 32 bits; false when the span has fewer left
    BGZF_HD bool get(int n, uint32_t &v)
    {
        if (cnt < n) refill();
        if (cnt < n) return false;
        v = (uint32_t)(buf & ((1ull << n) - 1));
        buf >>= n;
        cnt -= n;
        return true;
    }
};

// Canonical Huffman table from T.lens[base, base + n).  Returns INF_OK or INF_BAD_LENGTHS.  `lit`: the literal/length code,
// which must hold the end-of-block symbol.  As zlib does, an incomplete set is accepted only when it is a single code of
// length 1, and an all-zero distance set is accepted (a block of literals only).
template <class W> BGZF_HD inline int build(Tables &T, Huff &h, int base, int n, bool lit, const W &w)
{
    const uint8_t *lens = T.lens + base;
    if (w.lane() == 0) {
        for (int l = 0; l <= MAXBITS; ++l) h.count[l] = 0;
        for (int s = 0; s < n; ++s) h.count[lens[s]]++;
        h.offs[1] = 0;
        for (int l = 1; l < MAXBITS; ++l) h.offs[l + 1] = h.offs[l] + h.count[l];
        for (int s = 0; s < n; ++s)
            if (lens[s]) h.sorted[h.offs[lens[s]]++] = (uint16_t)s;
        h.offs[1] = 0;                               // (the placement advanced them)
        for (int l = 1; l < MAXBITS; ++l) h.offs[l + 1] = h.offs[l] + h.count[l];
    }
    for (int i = w.lane(); i < (1 << FAST); i += w.lanes()) h.fast[i] = 0;
    w.sync();
    int left = 1, coded = 0, maxlen = 0;
    for (int l = 1; l <= MAXBITS; ++l) {
        left = (left << 1) - h.count[l];
        if (left < 0) return INF_BAD_LENGTHS;                       // over-subscribed
        coded += h.count[l];
        if (h.count[l]) maxlen = l;
    }
    if (lit && lens[256] == 0) return INF_BAD_LENGTHS;
    if (left > 0 && !(coded == 0 && !lit) && !(coded == 1 && maxlen == 1)) return INF_BAD_LENGTHS;   // incomplete
    // the fast table: lane p takes the p-th symbol in canonical order; its code is first[len] + (p - offs[len])
    for (int p = w.lane(); p < coded; p += w.lanes()) {
        const int s = h.sorted[p], L = lens[s];
        if (L > FAST) continue;
        uint32_t first = 0;
        for (int l = 1; l < L; ++l) first = (first + h.count[l]) << 1;
        const uint32_t code = first + (uint32_t)(p - h.offs[L]);
        uint32_t rev = 0;
        for (int k = 0; k < L; ++k) rev |= ((code >> k) & 1u) << (L - 1 - k);
        for (uint32_t i = rev; i < (1u << FAST); i += 1u << L) h.fast[i] = (uint16_t)(s << 4 | L);
    }
    w.sync();
    return INF_OK;
}

// one symbol; -1 = invalid code or truncated stream
BGZF_HD inline int decode(const Huff &h, Bits &b)
{
    if (b.cnt < MAXBITS) b.refill();
    const uint16_t e = h.fast[b.buf & ((1u << FAST) - 1)];
    if (e) {
        const int L = e & 15;
        if (L > b.cnt) return -1;
        b.buf >>= L;
        b.cnt -= L;
        return e >> 4;
    }
    int code = 0, first = 0, index = 0;     // a code longer than FAST bits: the canonical walk, one bit at a time
    for (int L = 1; L <= MAXBITS; ++L) {
        if (b.cnt < 1) return -1;
        code |= (int)(b.buf & 1);
        b.buf >>= 1;
        b.cnt -= 1;
        const int count = h.count[L];
        if (code - count < first) return h.sorted[index + (code - first)];
        index += count;
        first = (first + count) << 1;
        code <<= 1;
    }
    return -1;
}

// the RFC 1951 base / extra-bit tables as formulas (no arrays: on the device an indexed local array lands in scratch)
BGZF_HD inline uint32_t len_base(int i) { return i < 8 ? (uint32_t)i + 3 : i == 28 ? 258u : ((4u + (i & 3)) << ((i - 4) >> 2)) + 3; }
BGZF_HD inline int len_extra(int i) { return i < 8 || i == 28 ? 0 : (i - 4) >> 2; }
BGZF_HD inline uint32_t dist_base(int i) { return i < 4 ? (uint32_t)i + 1 : (1u << (((i - 2) >> 1) + 1)) + 1 + ((uint32_t)(i & 1) << ((i - 2) >> 1)); }
BGZF_HD inline int dist_extra(int i) { return i < 4 ? 0 : (i - 2) >> 1; }
// the order in which the code-length code's lengths are sent: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
BGZF_HD inline int clen_order(int i) { return i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 7 - ((i - 5) >> 1) : 8 + ((i - 4) >> 1); }

template <class W> BGZF_HD inline int dynamic_tables(Tables &T, Bits &b, const W &w)
{
    uint32_t hlit, hdist, hclen;
    if (!b.get(5, hlit) || !b.get(5, hdist) || !b.get(4, hclen)) return INF_TRUNCATED;
    const int nlen = (int)hlit + 257, ndist = (int)hdist + 1, ncode = (int)hclen + 4;
    if (nlen > 286 || ndist > 30) return INF_BAD_LENGTHS;
    w.sync();                                       // every lane is done with the previous block's tables
    for (int i = w.lane(); i < NLIT + NDIST; i += w.lanes()) T.lens[i] = 0;
    w.sync();
    for (int i = 0; i < ncode; ++i) {
        uint32_t v;
        if (!b.get(3, v)) return INF_TRUNCATED;
        if (w.lane() == 0) T.lens[clen_order(i)] = (uint8_t)v;
    }
    w.sync();
    // the code-length code lives in the distance table's storage until the real one replaces it, and must be complete
    int rc = build(T, T.dist, 0, 19, false, w);
    if (rc) return rc;
    {
        int left = 1;
        for (int l = 1; l <= MAXBITS; ++l) left = (left << 1) - T.dist.count[l];
        if (left != 0) return INF_BAD_LENGTHS;
    }
    // decode() reads only the built table, so T.lens is free again: lane 0 writes the literal/length lengths to [0, nlen)
    // and the distance lengths to [NLIT, NLIT + ndist) (a repeat may run across the two)
    for (int i = w.lane(); i < 19; i += w.lanes()) T.lens[i] = 0;
    w.sync();
    uint32_t prev = 0;
    int idx = 0;
    while (idx < nlen + ndist) {
        const int sym = decode(T.dist, b);
        if (sym < 0) return INF_BAD_SYMBOL;
        uint32_t rep = 1, val = (uint32_t)sym, v = 0;
        if (sym == 16) {
            if (idx == 0) return INF_BAD_LENGTHS;
            if (!b.get(2, v)) return INF_TRUNCATED;
            val = prev;
            rep = 3 + v;
        } else if (sym == 17) {
            if (!b.get(3, v)) return INF_TRUNCATED;
            val = 0;
            rep = 3 + v;
        } else if (sym == 18) {
            if (!b.get(7, v)) return INF_TRUNCATED;
            val = 0;
            rep = 11 + v;
        }
        if (idx + (int)rep > nlen + ndist) return INF_BAD_LENGTHS;
        if (w.lane() == 0)
            for (uint32_t k = 0; k < rep; ++k, ++idx) T.lens[idx < nlen ? idx : NLIT + idx - nlen] = (uint8_t)val;
        else
            idx += (int)rep;
        prev = val;
    }
    w.sync();
    rc = build(T, T.lit, 0, nlen, true, w);
    if (rc) return rc;
    return build(T, T.dist, NLIT, ndist, false, w);
}

template <class W> BGZF_HD inline int fixed_tables(Tables &T, const W &w)
{
    w.sync();
    for (int i = w.lane(); i < NLIT + NDIST; i += w.lanes())
        T.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < NLIT ? 8 : 5;
    w.sync();
    const int rc = build(T, T.lit, 0, NLIT, true, w);
    return rc ? rc : build(T, T.dist, NLIT, NDIST, false, w);     // 30 and 31 decode, then fail as symbols
}

// Inflate the raw DEFLATE stream in[0, in_len) into out[0, out_cap).  *out_len = bytes produced (also on error).  Every
// lane of the wave calls this with the same arguments and gets the same result.
template <class W>
BGZF_HD inline int inflate_raw(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_cap, uint32_t *out_len,
                               Tables &T, const W &w)
{
    Bits b{in, in_len, 0, 0, 0};
    uint32_t o = 0;
    int rc = INF_OK;
    bool last = false;
    while (!last && rc == INF_OK) {
        uint32_t hdr;
        if (!b.get(3, hdr)) { rc = INF_TRUNCATED; break; }
        last = hdr & 1;
        const uint32_t type = hdr >> 1;
        if (type == 0) {                                            // stored
            b.buf >>= b.cnt & 7;
            b.cnt -= b.cnt & 7;
            uint32_t len, nlen;
            if (!b.get(16, len) || !b.get(16, nlen)) { rc = INF_TRUNCATED; break; }
            if (len != (~nlen & 0xffff)) { rc = INF_STORED_LEN; break; }
            const uint32_t at = b.pos - (uint32_t)(b.cnt >> 3);     // the bytes still in the bit buffer come first
            b.buf = 0;
            b.cnt = 0;
            if (len > in_len - at) { rc = INF_TRUNCATED; break; }
            if (len > out_cap - o) { rc = INF_OVERFLOW; break; }
            for (uint32_t k = (uint32_t)w.lane(); k < len; k += (uint32_t)w.lanes()) out[o + k] = in[at + k];
            b.pos = at + len;
            o += len;
            w.sync();
            continue;
        }
        if (type == 1) rc = fixed_tables(T, w);
        else if (type == 2) rc = dynamic_tables(T, b, w);
        else rc = INF_BAD_BLOCK_TYPE;
        if (rc) break;
        for (;;) {
            const int sym = decode(T.lit, b);
            if (sym < 0) { rc = INF_BAD_SYMBOL; break; }
            if (sym < 256) {
                if (o >= out_cap) { rc = INF_OVERFLOW; break; }
                if (w.lane() == 0) out[o] = (uint8_t)sym;
                ++o;
                continue;
            }
            if (sym == 256) break;
            const int li = sym - 257;
            if (li >= 29) { rc = INF_BAD_SYMBOL; break; }
            uint32_t v = 0;
            if (len_extra(li) && !b.get(len_extra(li), v)) { rc = INF_TRUNCATED; break; }
            const uint32_t len = len_base(li) + v;
            const int ds = decode(T.dist, b);
            if (ds < 0 || ds >= 30) { rc = INF_BAD_SYMBOL; break; }
            v = 0;
            if (dist_extra(ds) && !b.get(dist_extra(ds), v)) { rc = INF_TRUNCATED; break; }
            const uint32_t dist = dist_base(ds) + v;
            if (dist > o) { rc = INF_DISTANCE; break; }
            if (len > out_cap - o) { rc = INF_OVERFLOW; break; }
            // one piece never reads what it writes itself; a barrier makes each piece's stores visible to the next
            const uint32_t piece = w.lanes() == 1 ? len : (dist < (uint32_t)w.lanes() ? dist : (uint32_t)w.lanes());
            w.sync();
            for (uint32_t done = 0; done < len; done += piece) {
                const uint32_t n = len - done < piece ? len - done : piece;
                for (uint32_t k = (uint32_t)w.lane(); k < n; k += (uint32_t)w.lanes()) out[o + done + k] = out[o + done + k - dist];
                w.sync();
            }
            o += len;
        }
    }
    w.sync();
    *out_len = o;
    return rc;
}

}  // namespace bgzf

#if defined(__HIPCC__)
namespace bgzf {

struct DeviceWave {
    __device__ int lane() const { return (int)threadIdx.x; }
    __device__ int lanes() const { return 64; }
    __device__ void sync() const { __syncthreads(); }     // the workgroup is this one wave
};

// One workgroup (one wave) per BGZF block.  cdata_off / cdata_len: the raw DEFLATE span of block b in `comp`; out_off: where
// its ISIZE bytes go in `out`; status[b] = a Status.  The output of a block is only written within [out_off, out_off+isize).
__global__ __launch_bounds__(64) void inflate_blocks_kernel(const uint8_t *__restrict__ comp, const int64_t *cdata_off,
                                                            const int32_t *cdata_len, const uint32_t *isize,
                                                            const uint32_t *crc, const int64_t *out_off, uint8_t *out,
                                                            int32_t *status, int32_t n_blocks)
{
    __shared__ Tables T;
    __shared__ uint32_t scratch[65];
    const int blk = (int)blockIdx.x;
    if (blk >= n_blocks) return;
    DeviceWave w;
    fill_crc_table(T, w);
    uint8_t *dst = out + out_off[blk];
    uint32_t got = 0;
    int rc = inflate_raw(comp + cdata_off[blk], (uint32_t)cdata_len[blk], dst, isize[blk], &got, T, w);
    if (rc == INF_OK && got != isize[blk]) rc = INF_ISIZE;
    if (rc == INF_OK && crc32_wave(T, dst, got, w, scratch) != crc[blk]) rc = INF_CRC;
    if (threadIdx.x == 0) status[blk] = rc;
}

}  // namespace bgzf
#endif
