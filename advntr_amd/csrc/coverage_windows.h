// Covered bases per 100-bp reference window and the GC bins of those windows: the rule of CoverageBiasDetector
// (advntr/coverage_bias.py:38-91: get_covered_base_pairs_of_reference_windows, __add_bp_to_coverage_map,
// get_gc_content_coverage_map) with integer windows.  The cores are host + device code (BGZF_HD): the BAM pass runs them one
// thread per record, the host twins (advntr_coverage_windows_host, advntr_coverage_gc_host, advntr_coverage_bins_host) run the
// same code.
//
// The rule.
// - Every record counts, in file order: duplicates, secondary, supplementary, QC-fail and placed unmapped records included (the
//   reference filters none).  Which references count (a 'chr' prefix added when missing, then one of chr1-chr22, chrX, chrY) is
//   decided by the caller; here a reference either has windows or not.  A record with refID -1 (the reference raises on it) or
//   with a negative POS is skipped.
// - The interval is [pos, end): end = the CIGAR's reference end (M D N = X) when the record is mapped (no 0x4) and has a CIGAR,
//   else pos + l_seq (pysam: `reference_end or reference_start + len(seq)`).  Decided corners: a reference end of 0 (POS 0
//   and a CIGAR without reference bases) is falsy in the reference and gives pos + l_seq here too; a record with no reference
//   end and no SEQ (len(None) raises in the reference) gives the zero-length interval [pos, pos).
// - Windows w = pos / 100 through the last window the interval reaches ((end - 1) / 100; w0 itself when end == pos).  Window
//   [100w, 100w + 100) gains its overlap with the interval in bp and is present: a zero-length interval makes its own window
//   present with 0 bp.  Only full windows exist (w < len / 100); contributions past the last one are dropped, where the
//   reference raises KeyError.
// - Coverage = bp / 100; a present window with bp > 20000 (coverage above OUTLIER_COVERAGE = 200) is left out.
// - The GC bin of a window is gc / 10, gc = the number of *uppercase* 'G' and 'C' bytes of its 100 bases: get_gc_content on
//   the text get_chromosome_reference_sequence returns, with no upper().  Soft-masked (lower-case) bases do not count; the quirk
//   is kept.  int(gc / 100 * 10) == gc / 10 for every gc in 0..100, so the integer bin is the reference's.  Eleven bins (0..10).
// - Per bin: the number of windows and the sum of their bp, exact integers.
//
// The accumulation.  Per reference of n full windows, a difference array of n + 1 int64 slots; slot n is a sink for every add
// past the last full window.  One interval is at most four adds (first window, first interior window, last window, one past
// it) whose sum is zero, so every reference's slots sum to zero and one inclusive scan over the concatenated arrays of all
// references gives every window's bp.  A zero-length interval sets its window's bit in a presence bitmask; any other present
// window has bp > 0.  Adds are 64-bit integer atomics: the result does not depend on the order of the records, the chunking,
// or the run.
#pragma once
#include <stdint.h>

#include "bgzf_inflate.h"

namespace cov {

const int64_t WINDOW = 100;             // GC_CONTENT_WINDOW_SIZE
const int64_t OUTLIER_BP = 20000;       // OUTLIER_COVERAGE * WINDOW
const int BINS = 11;                    // gc / 10 for gc in 0..100

// end of the interval: ref_end = the CIGAR's reference end, or -1 when unmapped or without CIGAR (bam::reference_end)
BGZF_HD inline int64_t interval_end(int64_t pos, int64_t ref_end, int64_t l_seq)
{
    return ref_end > 0 ? ref_end : pos + l_seq;
}

// the difference-array adds of the interval [s, e) on a reference of n full windows: idx[k] (in 0..n, n = the sink) += val[k]
// for k < returned count.  *zero_window = the window a zero-length interval marks present, -1 otherwise (or when it is not a
// full window).  s >= 0, e >= s.
BGZF_HD inline int interval_adds(int64_t s, int64_t e, int64_t n, int64_t *idx, int64_t *val, int64_t *zero_window)
{
    const int64_t w0 = s / WINDOW;
    *zero_window = -1;
    if (e == s) {
        if (w0 < n) *zero_window = w0;
        return 0;
    }
    if (w0 >= n) return 0;
    const int64_t wl = (e - 1) / WINDOW;
    if (wl == w0) {
        idx[0] = w0; val[0] = e - s;
        idx[1] = w0 + 1 < n ? w0 + 1 : n; val[1] = -(e - s);
        return 2;
    }
    const int64_t x0 = WINDOW * (w0 + 1) - s, xl = e - WINDOW * wl;
    idx[0] = w0; val[0] = x0;
    idx[1] = w0 + 1 < n ? w0 + 1 : n; val[1] = WINDOW - x0;
    idx[2] = wl < n ? wl : n; val[2] = xl - WINDOW;
    idx[3] = wl + 1 < n ? wl + 1 : n; val[3] = -xl;
    return 4;
}

// GC count of the window starting at s[0]: uppercase G and C only
BGZF_HD inline int window_gc(const uint8_t *s)
{
    int g = 0;
    for (int i = 0; i < WINDOW; ++i) g += (s[i] == 'G') | (s[i] == 'C');
    return g;
}

// does window (bp, present) enter the bins
BGZF_HD inline bool counted(int64_t bp, bool present) { return present && bp <= OUTLIER_BP; }

}  // namespace cov

#if defined(__HIPCC__)
namespace cov {

// one thread per record of a chunk: the interval's adds into diff[base[ref] + idx] and the zero-length bit into zbits
// (bit (base[ref] + w) of a uint32 bitmask).  base[r] = -1: no windows (the reference has no full window).  A record whose
// parts overrun it is left to select_kernel, which reports it.
__global__ void accumulate_kernel(const uint8_t *buf, const int64_t *offs, int64_t n_rec, int32_t n_ref, const int64_t *base,
                                  const int64_t *n_windows, unsigned long long *diff, unsigned int *zbits)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec) return;
    bam::Record r;
    if (!bam::parse(buf, offs[i], r)) return;
    if (r.ref < 0 || r.ref >= n_ref || r.pos < 0 || base[r.ref] < 0) return;
    const int64_t e = interval_end(r.pos, bam::reference_end(buf, r), r.l_seq);
    int64_t idx[4], val[4], zw;
    const int k = interval_adds(r.pos, e, n_windows[r.ref], idx, val, &zw);
    const int64_t b = base[r.ref];
    for (int j = 0; j < k; ++j) atomicAdd(diff + b + idx[j], (unsigned long long)val[j]);
    if (zw >= 0) atomicOr(zbits + ((b + zw) >> 5), 1u << ((b + zw) & 31));
}

const int SCAN_THREADS = 256;
const int SCAN_ITEMS = 16;                                  // per thread: a tile is 4096 slots
const int64_t SCAN_TILE = (int64_t)SCAN_THREADS * SCAN_ITEMS;

__device__ inline int64_t block_inclusive_scan(int64_t v, int64_t *wave_sum, int64_t *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) wave_sum[wave] = x;
    __syncthreads();
    int64_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SCAN_THREADS / 64; ++w) {
        before += w < wave ? wave_sum[w] : 0;
        all += wave_sum[w];
    }
    *total = all;
    __syncthreads();
    return before + x;
}

// pass 1 of the scan: the sum of every tile of SCAN_TILE slots
__global__ void __launch_bounds__(SCAN_THREADS) tile_sums_kernel(const int64_t *diff, int64_t n, int64_t *tile_sum)
{
    __shared__ int64_t ws[SCAN_THREADS / 64];
    const int64_t at = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    int64_t s = 0;
    for (int k = 0; k < SCAN_ITEMS; ++k) s += at + k < n ? diff[at + k] : 0;
    int64_t total;
    (void)block_inclusive_scan(s, ws, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// pass 2: one workgroup turns the tile sums into exclusive prefixes, in place
__global__ void __launch_bounds__(SCAN_THREADS) tile_prefix_kernel(int64_t *tile_sum, int64_t n_tiles)
{
    __shared__ int64_t ws[SCAN_THREADS / 64];
    int64_t carry = 0;
    for (int64_t at = 0; at < n_tiles; at += SCAN_THREADS) {
        const int64_t j = at + threadIdx.x;
        const int64_t v = j < n_tiles ? tile_sum[j] : 0;
        int64_t total;
        const int64_t x = block_inclusive_scan(v, ws, &total);
        if (j < n_tiles) tile_sum[j] = carry + x - v;
        carry += total;
    }
}

// pass 3: every tile rescanned from its prefix; the diff array becomes the bp of every window, in place
__global__ void __launch_bounds__(SCAN_THREADS) tile_scan_kernel(int64_t *diff, int64_t n, const int64_t *tile_prefix)
{
    __shared__ int64_t ws[SCAN_THREADS / 64];
    const int64_t at = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    int64_t v[SCAN_ITEMS], s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        v[k] = at + k < n ? diff[at + k] : 0;
        s += v[k];
    }
    int64_t total;
    int64_t run = tile_prefix[blockIdx.x] + block_inclusive_scan(s, ws, &total) - s;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        run += v[k];
        if (at + k < n) diff[at + k] = run;
    }
}

const int GC_THREADS = 256;

// one thread per full window of a chromosome: its uppercase G/C count
__global__ void gc_kernel(const uint8_t *chrom, int64_t n_windows, uint8_t *gc)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_windows) return;
    gc[w] = (uint8_t)window_gc(chrom + WINDOW * w);
}

const int BIN_THREADS = 256;
const int BIN_ITEMS = 16;                                   // windows per thread

// windows [0, n) of one reference (bp, presence bits from bit `zbit0` on, gc or NULL = every window in bin 0): per bin the
// number of counted windows and their bp.  Each thread keeps its own eleven pairs in registers (static indices), a wave sums
// them with shuffles, the waves of a workgroup in LDS, then one 64-bit atomic per workgroup and bin.
__global__ void __launch_bounds__(BIN_THREADS) bins_kernel(const int64_t *bp, const unsigned int *zbits, int64_t zbit0,
                                                           const uint8_t *gc, int64_t n, unsigned long long *bin_windows,
                                                           unsigned long long *bin_bp)
{
    __shared__ unsigned long long s_w[BINS], s_bp[BINS];
    if (threadIdx.x < BINS) { s_w[threadIdx.x] = 0; s_bp[threadIdx.x] = 0; }
    __syncthreads();
    int64_t c[BINS], t[BINS];
#pragma unroll
    for (int j = 0; j < BINS; ++j) { c[j] = 0; t[j] = 0; }
    // consecutive threads take consecutive windows: item k of thread x is window base + k * BIN_THREADS + x
    const int64_t base = (int64_t)blockIdx.x * BIN_THREADS * BIN_ITEMS + threadIdx.x;
    for (int k = 0; k < BIN_ITEMS; ++k) {
        const int64_t w = base + (int64_t)k * BIN_THREADS;
        if (w >= n) break;
        const int64_t b = bp[w], z = zbit0 + w;
        const bool present = b > 0 || ((zbits[z >> 5] >> (z & 31)) & 1u);
        if (!counted(b, present)) continue;
        const int bin = gc ? gc[w] / 10 : 0;
#pragma unroll
        for (int j = 0; j < BINS; ++j) {
            c[j] += j == bin;
            t[j] += j == bin ? b : 0;
        }
    }
#pragma unroll
    for (int j = 0; j < BINS; ++j) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            c[j] += __shfl_xor(c[j], d, 64);
            t[j] += __shfl_xor(t[j], d, 64);
        }
    }
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int j = 0; j < BINS; ++j)
            if (c[j]) {
                atomicAdd(&s_w[j], (unsigned long long)c[j]);
                atomicAdd(&s_bp[j], (unsigned long long)t[j]);
            }
    __syncthreads();
    if (threadIdx.x < BINS && s_w[threadIdx.x]) {
        atomicAdd(bin_windows + threadIdx.x, s_w[threadIdx.x]);
        atomicAdd(bin_bp + threadIdx.x, s_bp[threadIdx.x]);
    }
}

}  // namespace cov
#endif
