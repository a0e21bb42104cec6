// advntr_genome_scan / advntr_genome_scan_host: the false reads of many loci on one chromosome (csrc/genome_scan.h).
//
// The device pass walks the chromosome in ordered chunks.  A 4^11-bit membership bitset of the live loci's keywords (512 KiB,
// L2-resident) answers "is this 11-mer a keyword of anyone"; each thread slides a 2-bit window over a stripe of 64 positions
// read as six 16-byte loads.  A chunk is counted first (per-thread counts, per-block totals, one scan of the totals), then
// only the threads that hold a hit walk their stripe again and write (position, 11-mer) in position order, so nothing is
// dropped and the output is sized from the count.  The host folds the hits into the loci through a direct owner index
// (11-mer -> loci) in chromosome order; a locus that reaches the cap leaves the live set and the bitset of the next chunk.
// Included by engine.hip (after abi_bam.h: DevBuf, g_cache, current_device).
#include "genome_scan.h"

namespace {

const int GS_THREADS = 256;
const int GS_STRIPE = 64;                               // positions per thread
const int GS_PAD = 128;                                 // 'N' bytes either side of the device copy
const int64_t GS_CHUNK = (int64_t)1 << 24;              // positions per chunk
const int GS_SCAN_THREADS = 1024;

// the loci of one call: keyword owners (CSR over all 4^11 11-mers) and the bitset of the live loci's keywords
struct ScanLoci {
    std::vector<int32_t> head, owner;
    std::vector<uint32_t> bits;
    std::vector<std::vector<uint32_t>> kmers;           // per locus, distinct
};

int scan_loci(const char *who, int32_t n_loci, const int32_t *kw_off, const uint32_t *kw, ScanLoci &S)
{
    if (n_loci < 0 || (n_loci && !kw_off) || (n_loci && kw_off[n_loci] > 0 && !kw))
        return fail(ADVNTR_ERR_ARG, "%s: bad loci", who);
    S.kmers.assign((size_t)n_loci, {});
    S.head.assign((size_t)gscan::N_KMERS + 1, 0);
    for (int32_t L = 0; L < n_loci; ++L) {
        if (kw_off[L + 1] < kw_off[L]) return fail(ADVNTR_ERR_ARG, "%s: keyword offsets of locus %d decrease", who, (int)L);
        std::vector<uint32_t> &k = S.kmers[L];
        k.assign(kw + kw_off[L], kw + kw_off[L + 1]);
        for (uint32_t v : k)
            if (v > gscan::KMER_MASK) return fail(ADVNTR_ERR_ARG, "%s: keyword value %u of locus %d is not an 11-mer", who, v, (int)L);
        std::sort(k.begin(), k.end());
        k.erase(std::unique(k.begin(), k.end()), k.end());
        for (uint32_t v : k) ++S.head[v + 1];
    }
    for (int64_t v = 0; v < gscan::N_KMERS; ++v) S.head[v + 1] += S.head[v];
    S.owner.assign((size_t)S.head[gscan::N_KMERS], 0);
    std::vector<int32_t> at(S.head.begin(), S.head.end() - 1);
    for (int32_t L = 0; L < n_loci; ++L)                 // owners of an 11-mer in locus order
        for (uint32_t v : S.kmers[L]) S.owner[at[v]++] = L;
    return ADVNTR_OK;
}

void scan_bits(const ScanLoci &S, const std::vector<gscan::LocusState> &st, std::vector<uint32_t> &bits)
{
    bits.assign((size_t)(gscan::N_KMERS / 32), 0u);
    for (size_t L = 0; L < st.size(); ++L)
        if (st[L].live)
            for (uint32_t v : S.kmers[L]) bits[v >> 5] |= 1u << (v & 31);
}

// the per-locus fold of the hits, in chromosome order
struct ScanFold {
    const ScanLoci &S;
    const uint8_t *s;
    int64_t n;
    const int64_t *vs, *ve;
    int64_t *rb, *re;
    std::vector<gscan::LocusState> st;
    int32_t live;
    bool capped = false;                                 // a locus stopped since the last bitset

    ScanFold(const ScanLoci &S_, const uint8_t *s_, int64_t n_, int32_t n_loci, const int64_t *vs_, const int64_t *ve_,
             int64_t *rb_, int64_t *re_)
        : S(S_), s(s_), n(n_), vs(vs_), ve(ve_), rb(rb_), re(re_), st((size_t)n_loci), live(n_loci)
    {
        for (auto &x : st) gscan::locus_init(x);
    }

    void hit(int64_t i, uint32_t kmer)
    {
        for (int32_t k = S.head[kmer]; k < S.head[kmer + 1]; ++k) {
            const int32_t L = S.owner[k];
            gscan::LocusState &x = st[L];
            if (!x.live) continue;
            gscan::locus_hit(x, i, s, n, vs[L], ve[L], rb + (int64_t)L * gscan::READ_CAPACITY, re + (int64_t)L * gscan::READ_CAPACITY);
            if (!x.live) { --live; capped = true; }
        }
    }

    void counts(int32_t *n_reads) const
    {
        for (size_t L = 0; L < st.size(); ++L) n_reads[L] = st[L].reads;
    }
};

__device__ inline int gs_block_exclusive_scan(int v, int *wave_sum, int *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) wave_sum[wave] = x;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < GS_THREADS / 64; ++w) {
        before += w < wave ? wave_sum[w] : 0;
        all += wave_sum[w];
    }
    *total = all;
    return before + x - v;
}

// the stripe of positions [p0, p0 + GS_STRIPE) ∩ [.., hi): bases [p0-1, p0+GS_STRIPE+K-1) pushed through the window; s points
// at base 0 of a copy with GS_PAD 'N' bytes either side, p0 a multiple of GS_STRIPE
template <class F>
__device__ inline void gs_stripe(const uint8_t *s, int64_t n, int64_t p0, int64_t hi, const uint32_t *bits, F on_hit)
{
    const uint4 *src = reinterpret_cast<const uint4 *>(s + p0 - 16);
    uint32_t w[24];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const uint4 v = src[k];
        w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
    }
    gscan::Window win;
    gscan::window_init(win);
#pragma unroll
    for (int t = 15; t < 16 + GS_STRIPE + gscan::K - 1; ++t) {       // byte p0 - 16 + t
        gscan::window_push(win, (uint8_t)(w[t >> 2] >> (8 * (t & 3))));
        const int64_t i = p0 - 16 + t - gscan::K + 1;
        if (t >= 16 + gscan::K - 1 && gscan::window_ready(win) && i < hi && gscan::position_in_range(i, n) &&
            ((bits[win.value >> 5] >> (win.value & 31)) & 1u))
            on_hit(i, win.value);
    }
}

__global__ __launch_bounds__(GS_THREADS) void gs_count_kernel(const uint8_t *s, int64_t n, int64_t lo, int64_t hi,
                                                              const uint32_t *bits, int32_t *thread_count, int32_t *block_count)
{
    __shared__ int wave_sum[GS_THREADS / 64];
    const int64_t t = (int64_t)blockIdx.x * GS_THREADS + threadIdx.x;
    const int64_t p0 = lo + t * GS_STRIPE;
    int c = 0;
    if (p0 < hi) gs_stripe(s, n, p0, hi, bits, [&](int64_t, uint32_t) { ++c; });
    thread_count[t] = c;
    int total;
    gs_block_exclusive_scan(c, wave_sum, &total);
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

// exclusive scan of n block counts by one workgroup; the sum goes to *total
__global__ __launch_bounds__(GS_SCAN_THREADS) void gs_scan_blocks_kernel(const int32_t *count, int32_t n, int64_t *offset,
                                                                         int64_t *total)
{
    __shared__ int64_t part[GS_SCAN_THREADS];
    __shared__ int64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int32_t base = 0; base < n; base += GS_SCAN_THREADS) {
        const int32_t k = base + threadIdx.x;
        const int64_t v = k < n ? count[k] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < GS_SCAN_THREADS; d <<= 1) {
            const int64_t y = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
            __syncthreads();
            part[threadIdx.x] += y;
            __syncthreads();
        }
        if (k < n) offset[k] = carry + part[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == GS_SCAN_THREADS - 1) carry += part[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(GS_THREADS) void gs_write_kernel(const uint8_t *s, int64_t n, int64_t lo, int64_t hi,
                                                              const uint32_t *bits, const int32_t *thread_count,
                                                              const int64_t *block_offset, uint64_t *hits)
{
    __shared__ int wave_sum[GS_THREADS / 64];
    const int64_t t = (int64_t)blockIdx.x * GS_THREADS + threadIdx.x;
    const int64_t p0 = lo + t * GS_STRIPE;
    const int c = thread_count[t];
    int total;
    int64_t at = block_offset[blockIdx.x] + gs_block_exclusive_scan(c, wave_sum, &total);
    if (c == 0 || p0 >= hi) return;
    gs_stripe(s, n, p0, hi, bits, [&](int64_t i, uint32_t v) { hits[at++] = ((uint64_t)i << (2 * gscan::K)) | v; });
}

int scan_args(const char *who, const uint8_t *s, int64_t n, int32_t n_loci, const int64_t *vs, const int64_t *ve,
              int64_t *rb, int64_t *re, int32_t *n_reads)
{
    if ((n && !s) || n < 0 || n_loci < 0 || (n_loci && (!vs || !ve || !rb || !re || !n_reads)))
        return fail(ADVNTR_ERR_ARG, "%s: bad argument", who);
    if (n >= ((int64_t)1 << (64 - 2 * gscan::K - 1)))
        return fail(ADVNTR_ERR_ARG, "%s: chromosome of %lld bases is too long", who, (long long)n);
    return ADVNTR_OK;
}

}  // namespace

extern "C" int advntr_genome_scan_host(const uint8_t *chrom, int64_t n, int32_t n_loci, const int64_t *vntr_start,
                                       const int64_t *vntr_end, const int32_t *kw_off, const uint32_t *kw, int64_t *read_begin,
                                       int64_t *read_end, int32_t *n_reads)
{
    const char *who = "advntr_genome_scan_host";
    if (scan_args(who, chrom, n, n_loci, vntr_start, vntr_end, read_begin, read_end, n_reads)) return ADVNTR_ERR_ARG;
    ScanLoci S;
    if (int rc = scan_loci(who, n_loci, kw_off, kw, S)) return rc;
    ScanFold F(S, chrom, n, n_loci, vntr_start, vntr_end, read_begin, read_end);
    gscan::Window w;
    gscan::window_init(w);
    for (int64_t q = 0; q < n && F.live > 0; ++q) {
        gscan::window_push(w, chrom[q]);
        const int64_t i = q - gscan::K + 1;
        if (gscan::window_ready(w) && gscan::position_in_range(i, n) && S.head[w.value + 1] > S.head[w.value]) F.hit(i, w.value);
    }
    F.counts(n_reads);
    return ADVNTR_OK;
}

extern "C" int advntr_genome_scan(const uint8_t *chrom, int64_t n, int32_t n_loci, const int64_t *vntr_start,
                                  const int64_t *vntr_end, const int32_t *kw_off, const uint32_t *kw, int64_t chunk,
                                  int64_t *read_begin, int64_t *read_end, int32_t *n_reads, double *stats)
{
    const char *who = "advntr_genome_scan";
    if (scan_args(who, chrom, n, n_loci, vntr_start, vntr_end, read_begin, read_end, n_reads)) return ADVNTR_ERR_ARG;
    if (chunk < 0) return fail(ADVNTR_ERR_ARG, "%s: negative chunk", who);
    chunk = chunk ? (chunk + GS_STRIPE - 1) / GS_STRIPE * GS_STRIPE : GS_CHUNK;
    if (advntr_device_count() <= 0) return fail(ADVNTR_ERR_DEVICE, "%s: no HIP device visible (no CPU fallback)", who);
    double st[ADVNTR_GENOME_SCAN_STATS] = {0};
    const auto t_all = std::chrono::steady_clock::now();
    ScanLoci S;
    if (int rc = scan_loci(who, n_loci, kw_off, kw, S)) return rc;
    ScanFold F(S, chrom, n, n_loci, vntr_start, vntr_end, read_begin, read_end);
    const int64_t end = std::max<int64_t>(n - gscan::K, 0);          // positions i < n - K
    if (F.live > 0 && end > 1) {
        const int dev = current_device();
        hipStream_t strm = g_cache.get_stream(dev);
        if (!strm) return fail(ADVNTR_ERR_DEVICE, "%s: no stream", who);
        hipEvent_t ev[4];
        for (auto &e : ev) e = g_cache.get_event(dev);
        struct Back {
            int dev; hipStream_t s; hipEvent_t *ev;
            ~Back() { for (int k = 0; k < 4; ++k) if (ev[k]) g_cache.put_event(dev, ev[k]); g_cache.put_stream(dev, s); }
        } back{dev, strm, ev};
        for (auto &e : ev)
            if (!e) return fail(ADVNTR_ERR_DEVICE, "%s: no event", who);
        const int64_t max_threads = (chunk + GS_STRIPE - 1) / GS_STRIPE;
        const int64_t max_blocks = (max_threads + GS_THREADS - 1) / GS_THREADS;
        if (max_blocks > INT32_MAX) return fail(ADVNTR_ERR_ARG, "%s: chunk too large", who);
        DevBuf<uint8_t> d_s;
        DevBuf<uint32_t> d_bits;
        DevBuf<int32_t> d_tcount, d_bcount;
        DevBuf<int64_t> d_boff, d_total;
        DevBuf<uint64_t> d_hits;
        if (d_s.ensure((size_t)n + 2 * GS_PAD) || d_bits.ensure((size_t)(gscan::N_KMERS / 32)) ||
            d_tcount.ensure((size_t)(max_blocks * GS_THREADS)) || d_bcount.ensure((size_t)max_blocks) ||
            d_boff.ensure((size_t)max_blocks) || d_total.ensure(1))
            return ADVNTR_ERR_DEVICE;
        const auto t_up = std::chrono::steady_clock::now();
        HIP_TRY(hipMemsetAsync(d_s.p, 'N', GS_PAD, strm));
        HIP_TRY(hipMemsetAsync(d_s.p + GS_PAD + n, 'N', GS_PAD, strm));
        HIP_TRY(hipMemcpyAsync(d_s.p + GS_PAD, chrom, (size_t)n, hipMemcpyHostToDevice, strm));
        scan_bits(S, F.st, S.bits);
        HIP_TRY(hipMemcpyAsync(d_bits.p, S.bits.data(), S.bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice, strm));
        HIP_TRY(hipStreamSynchronize(strm));
        st[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_up).count();
        const uint8_t *s = d_s.p + GS_PAD;
        std::vector<uint64_t> h_hits;
        for (int64_t lo = 0; lo < end && F.live > 0; lo += chunk) {
            const int64_t hi = std::min(lo + chunk, end);
            const int32_t blocks = (int32_t)(((hi - lo + GS_STRIPE - 1) / GS_STRIPE + GS_THREADS - 1) / GS_THREADS);
            if (F.capped) {                              // loci that stopped leave the bitset
                scan_bits(S, F.st, S.bits);
                HIP_TRY(hipMemcpyAsync(d_bits.p, S.bits.data(), S.bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice, strm));
                F.capped = false;
            }
            HIP_TRY(hipEventRecord(ev[0], strm));
            hipLaunchKernelGGL(gs_count_kernel, dim3(blocks), dim3(GS_THREADS), 0, strm, s, n, lo, hi, d_bits.p, d_tcount.p,
                               d_bcount.p);
            hipLaunchKernelGGL(gs_scan_blocks_kernel, dim3(1), dim3(GS_SCAN_THREADS), 0, strm, d_bcount.p, blocks, d_boff.p,
                               d_total.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(ev[1], strm));
            int64_t total = 0;
            HIP_TRY(hipMemcpyAsync(&total, d_total.p, sizeof total, hipMemcpyDeviceToHost, strm));
            HIP_TRY(hipStreamSynchronize(strm));
            if (total < 0 || total > (hi - lo)) return fail(ADVNTR_ERR_DEVICE, "%s: hit count %lld out of range", who, (long long)total);
            HIP_TRY(hipEventRecord(ev[2], strm));
            if (total) {
                if (d_hits.ensure((size_t)total)) return ADVNTR_ERR_DEVICE;
                hipLaunchKernelGGL(gs_write_kernel, dim3(blocks), dim3(GS_THREADS), 0, strm, s, n, lo, hi, d_bits.p, d_tcount.p,
                                   d_boff.p, d_hits.p);
                HIP_TRY(hipGetLastError());
            }
            HIP_TRY(hipEventRecord(ev[3], strm));
            h_hits.resize((size_t)total);
            if (total) HIP_TRY(hipMemcpyAsync(h_hits.data(), d_hits.p, (size_t)total * sizeof(uint64_t), hipMemcpyDeviceToHost, strm));
            HIP_TRY(hipStreamSynchronize(strm));
            float ms_count = 0.f, ms_write = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms_count, ev[0], ev[1]));
            HIP_TRY(hipEventElapsedTime(&ms_write, ev[2], ev[3]));
            st[1] += ms_count + ms_write;
            st[3] += (double)total;
            st[4] += 1;
            st[5] += (double)(std::min(hi + gscan::K, n) - std::max<int64_t>(lo - 1, 0));
            const auto t_fold = std::chrono::steady_clock::now();
            for (int64_t k = 0; k < total && F.live > 0; ++k)
                F.hit((int64_t)(h_hits[k] >> (2 * gscan::K)), (uint32_t)(h_hits[k] & gscan::KMER_MASK));
            st[2] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_fold).count();
        }
    }
    F.counts(n_reads);
    st[6] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_all).count();
    if (stats)
        for (int k = 0; k < ADVNTR_GENOME_SCAN_STATS; ++k) stats[k] = st[k];
    return ADVNTR_OK;
}
