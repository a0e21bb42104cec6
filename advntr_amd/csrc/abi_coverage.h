// C-ABI entry points of the coverage windows (coverage_windows.h): the host twins of the accumulation, the GC count and the
// binning, the device GC count, and the per-window fetch and device binning of an ADVNTR_BAM_COVERAGE pass.  Included by
// engine.hip after abi_bam.h (BamCoverage, DevBuf, current_device).

extern "C" int advntr_coverage_windows_host(int32_t n_ref, const int64_t *n_windows, const int32_t *rec_ref, const int64_t *rec_start,
                                            const int64_t *rec_end, int64_t n_rec, int64_t *bp, uint8_t *present)
{
    if (n_ref < 0 || n_rec < 0 || (n_ref && !n_windows) || (n_rec && (!rec_ref || !rec_start || !rec_end)) || !bp || !present)
        return fail(ADVNTR_ERR_ARG, "advntr_coverage_windows_host: bad argument");
    std::vector<int64_t> base((size_t)n_ref + 1, 0);
    for (int32_t r = 0; r < n_ref; ++r) {
        if (n_windows[r] < 0) return fail(ADVNTR_ERR_ARG, "advntr_coverage_windows_host: negative window count of reference %d", (int)r);
        base[r + 1] = base[r] + n_windows[r] + 1;           // one sink slot per reference, as on the device
    }
    std::vector<int64_t> diff((size_t)base[n_ref], 0);
    std::vector<uint8_t> zero((size_t)base[n_ref], 0);
    for (int64_t i = 0; i < n_rec; ++i) {
        const int32_t r = rec_ref[i];
        if (r < 0 || r >= n_ref || rec_start[i] < 0 || !n_windows[r]) continue;
        if (rec_end[i] < rec_start[i])
            return fail(ADVNTR_ERR_ARG, "advntr_coverage_windows_host: interval %lld ends before it starts", (long long)i);
        int64_t idx[4], val[4], zw;
        const int k = cov::interval_adds(rec_start[i], rec_end[i], n_windows[r], idx, val, &zw);
        for (int j = 0; j < k; ++j) diff[base[r] + idx[j]] += val[j];
        if (zw >= 0) zero[base[r] + zw] = 1;
    }
    int64_t out = 0;
    for (int32_t r = 0; r < n_ref; ++r) {
        int64_t run = 0;
        for (int64_t w = 0; w < n_windows[r]; ++w, ++out) {
            run += diff[base[r] + w];
            bp[out] = run;
            present[out] = run > 0 || zero[base[r] + w];
        }
    }
    return ADVNTR_OK;
}

extern "C" int advntr_coverage_gc_host(const uint8_t *chrom, int64_t n, uint8_t *gc)
{
    if (n < 0 || (n >= cov::WINDOW && (!chrom || !gc))) return fail(ADVNTR_ERR_ARG, "advntr_coverage_gc_host: bad argument");
    for (int64_t w = 0; w < n / cov::WINDOW; ++w) gc[w] = (uint8_t)cov::window_gc(chrom + cov::WINDOW * w);
    return ADVNTR_OK;
}

extern "C" int advntr_coverage_bins_host(const int64_t *bp, const uint8_t *present, const uint8_t *gc, int64_t n_windows,
                                         int64_t *bin_windows, int64_t *bin_bp)
{
    if (n_windows < 0 || (n_windows && (!bp || !present)) || !bin_windows || !bin_bp)
        return fail(ADVNTR_ERR_ARG, "advntr_coverage_bins_host: bad argument");
    for (int64_t w = 0; w < n_windows; ++w) {
        if (!cov::counted(bp[w], present[w] != 0)) continue;
        const int bin = gc ? gc[w] / 10 : 0;
        if (bin >= cov::BINS) return fail(ADVNTR_ERR_ARG, "advntr_coverage_bins_host: GC count %d of window %lld above 100", gc[w], (long long)w);
        bin_windows[bin] += 1;
        bin_bp[bin] += bp[w];
    }
    return ADVNTR_OK;
}

namespace {

// chrom[n] to the device and its GC counts into d_gc (n / 100 windows); ms[0] += upload, ms[1] += kernel
static int coverage_gc_device(const uint8_t *chrom, int64_t n, DevBuf<uint8_t> &d_chrom, DevBuf<uint8_t> &d_gc, double *ms)
{
    const int64_t nw = n / cov::WINDOW;
    int rc;
    if ((rc = d_chrom.ensure((size_t)std::max<int64_t>(1, nw * cov::WINDOW))) || (rc = d_gc.ensure((size_t)std::max<int64_t>(1, nw))))
        return rc;
    if (!nw) return ADVNTR_OK;
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    struct Events {
        hipEvent_t *e;
        ~Events() { for (int i = 0; i < 3; ++i) if (e[i]) (void)hipEventDestroy(e[i]); }
    } guard{e};
    for (int i = 0; i < 3; ++i) HIP_TRY(hipEventCreate(&e[i]));
    HIP_TRY(hipEventRecord(e[0], nullptr));
    HIP_TRY(hipMemcpy(d_chrom.p, chrom, (size_t)(nw * cov::WINDOW), hipMemcpyHostToDevice));     // the full windows only
    HIP_TRY(hipEventRecord(e[1], nullptr));
    hipLaunchKernelGGL(cov::gc_kernel, dim3((unsigned)((nw + cov::GC_THREADS - 1) / cov::GC_THREADS)), dim3(cov::GC_THREADS), 0, nullptr,
                       d_chrom.p, nw, d_gc.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e[2], nullptr));
    HIP_TRY(hipEventSynchronize(e[2]));
    float a = 0, b = 0;
    HIP_TRY(hipEventElapsedTime(&a, e[0], e[1]));
    HIP_TRY(hipEventElapsedTime(&b, e[1], e[2]));
    ms[0] += a;
    ms[1] += b;
    return ADVNTR_OK;
}

}  // namespace

extern "C" int advntr_coverage_gc(const uint8_t *chrom, int64_t n, uint8_t *gc, double *ms)
{
    if (n < 0 || (n >= cov::WINDOW && (!chrom || !gc))) return fail(ADVNTR_ERR_ARG, "advntr_coverage_gc: bad argument");
    if (advntr_device_count() <= 0) return fail(ADVNTR_ERR_DEVICE, "advntr_coverage_gc: no HIP device visible (no CPU fallback)");
    (void)current_device();
    DevBuf<uint8_t> d_chrom, d_gc;
    double t[2] = {0, 0};
    int rc = coverage_gc_device(chrom, n, d_chrom, d_gc, t);
    if (rc) return rc;
    const int64_t nw = n / cov::WINDOW;
    if (nw) HIP_TRY(hipMemcpy(gc, d_gc.p, (size_t)nw, hipMemcpyDeviceToHost));
    if (ms) { ms[0] = t[0]; ms[1] = t[1]; }
    return ADVNTR_OK;
}

extern "C" int advntr_bam_coverage_info(const advntr_bam_kept *K, int32_t *n_ref, int64_t *n_windows, double *stats)
{
    if (!K) return fail(ADVNTR_ERR_ARG, "advntr_bam_coverage_info: null handle");
    if (!K->cov.on) return fail(ADVNTR_ERR_ARG, "advntr_bam_coverage_info: the pass ran without ADVNTR_BAM_COVERAGE");
    if (n_ref) *n_ref = (int32_t)K->cov.n_windows.size();
    if (n_windows) std::copy(K->cov.n_windows.begin(), K->cov.n_windows.end(), n_windows);
    if (stats) std::copy(K->cov.stats, K->cov.stats + ADVNTR_BAM_COVERAGE_STATS, stats);
    return ADVNTR_OK;
}

extern "C" int advntr_bam_coverage_windows(const advntr_bam_kept *K, int32_t ref, int64_t *bp, uint8_t *present)
{
    if (!K || !bp || !present) return fail(ADVNTR_ERR_ARG, "advntr_bam_coverage_windows: bad argument");
    const BamCoverage &C = K->cov;
    if (!C.on) return fail(ADVNTR_ERR_ARG, "advntr_bam_coverage_windows: the pass ran without ADVNTR_BAM_COVERAGE");
    if (ref < 0 || ref >= (int32_t)C.n_windows.size()) return fail(ADVNTR_ERR_ARG, "advntr_bam_coverage_windows: no reference %d", (int)ref);
    const int64_t n = C.n_windows[ref];
    if (!n) return ADVNTR_OK;
    (void)current_device();
    const int64_t b = C.base[ref];
    HIP_TRY(hipMemcpy(bp, C.d_diff.p + b, (size_t)n * 8, hipMemcpyDeviceToHost));
    // the presence bits of [b, b + n): the words that hold them, then bit by bit
    const int64_t w0 = b / 32, w1 = (b + n + 31) / 32;
    std::vector<uint32_t> words((size_t)(w1 - w0));
    HIP_TRY(hipMemcpy(words.data(), C.d_zbits.p + w0, words.size() * 4, hipMemcpyDeviceToHost));
    for (int64_t w = 0; w < n; ++w) {
        const int64_t z = b + w - 32 * w0;
        present[w] = bp[w] > 0 || ((words[z >> 5] >> (z & 31)) & 1u);
    }
    return ADVNTR_OK;
}

extern "C" int advntr_bam_coverage_bins(advntr_bam_kept *K, int32_t ref, const uint8_t *chrom, int64_t chrom_len, int64_t *bin_windows,
                                        int64_t *bin_bp)
{
    const char *who = "advntr_bam_coverage_bins";
    if (!K || !bin_windows || !bin_bp || chrom_len < 0) return fail(ADVNTR_ERR_ARG, "%s: bad argument", who);
    BamCoverage &C = K->cov;
    if (!C.on) return fail(ADVNTR_ERR_ARG, "%s: the pass ran without ADVNTR_BAM_COVERAGE", who);
    if (ref < 0 || ref >= (int32_t)C.n_windows.size()) return fail(ADVNTR_ERR_ARG, "%s: no reference %d", who, (int)ref);
    const int64_t n = C.n_windows[ref];
    if (chrom && chrom_len / cov::WINDOW != n)
        return fail(ADVNTR_ERR_ARG, "%s: reference %d has %lld full windows in the BAM header, the sequence given has %lld", who, (int)ref,
                    (long long)n, (long long)(chrom_len / cov::WINDOW));
    if (!n) return ADVNTR_OK;
    (void)current_device();
    DevBuf<uint8_t> d_chrom, d_gc;
    int rc;
    if (chrom && (rc = coverage_gc_device(chrom, chrom_len, d_chrom, d_gc, C.stats + 2))) return rc;
    DevBuf<unsigned long long> d_bins;
    if ((rc = d_bins.ensure(2 * cov::BINS))) return rc;
    HIP_TRY(hipMemset(d_bins.p, 0, 2 * cov::BINS * 8));
    hipEvent_t e[2] = {nullptr, nullptr};
    struct Events {
        hipEvent_t *e;
        ~Events() { for (int i = 0; i < 2; ++i) if (e[i]) (void)hipEventDestroy(e[i]); }
    } guard{e};
    for (int i = 0; i < 2; ++i) HIP_TRY(hipEventCreate(&e[i]));
    const int64_t per_block = (int64_t)cov::BIN_THREADS * cov::BIN_ITEMS;
    HIP_TRY(hipEventRecord(e[0], nullptr));
    hipLaunchKernelGGL(cov::bins_kernel, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(cov::BIN_THREADS), 0, nullptr,
                       C.d_diff.p + C.base[ref], C.d_zbits.p, C.base[ref], chrom ? d_gc.p : (const uint8_t *)nullptr, n, d_bins.p,
                       d_bins.p + cov::BINS);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e[1], nullptr));
    unsigned long long h[2 * cov::BINS];
    HIP_TRY(hipMemcpy(h, d_bins.p, sizeof h, hipMemcpyDeviceToHost));       // the eleven pairs only
    HIP_TRY(hipEventSynchronize(e[1]));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e[0], e[1]));
    C.stats[4] += ms;
    for (int j = 0; j < cov::BINS; ++j) {
        bin_windows[j] += (int64_t)h[j];
        bin_bp[j] += (int64_t)h[cov::BINS + j];
    }
    return ADVNTR_OK;
}
