// abi_bam.h -- C-ABI entry points of the BAM input (bgzf_inflate.h, bam_records.h).  Included by engine.hip.
#pragma once
#include <cstdio>
#include <functional>
#include <tuple>
#include "bgzf_inflate.h"
#include "bam_records.h"
#include "bam_spans.h"
#include "coverage_windows.h"

namespace {

struct BgzfBlock {
    int64_t off;            // file offset of the block
    int64_t cdata;          // file offset of the raw DEFLATE data
    int32_t bytes, clen;    // BSIZE + 1; DEFLATE bytes
    uint32_t crc, isize;
};

// Frame one block at data[at, n).  0 = ok, 1 = fewer bytes than the block (truncated, or the rest of a buffer), -1 = not BGZF
// (message in *why).  BGZF: a gzip member with FEXTRA whose extra field holds the subfield BC (SLEN 2) = BSIZE.
static int frame_block(const uint8_t *data, int64_t n, int64_t at, BgzfBlock &b, const char **why)
{
    const uint8_t *p = data + at;
    const int64_t left = n - at;
    if (left < 18) return 1;
    if (p[0] != 31 || p[1] != 139 || p[2] != 8) { *why = "not a gzip member"; return -1; }
    if (!(p[3] & 4)) { *why = "gzip member without the BC extra field (plain gzip, not BGZF)"; return -1; }
    const int64_t xlen = bam::rd_u16(p + 10);
    if (left < 12 + xlen) return 1;
    int64_t bsize = -1;
    for (int64_t x = 0; x + 4 <= xlen;) {
        const int64_t slen = bam::rd_u16(p + 12 + x + 2);
        if (p[12 + x] == 66 && p[12 + x + 1] == 67 && slen == 2 && x + 6 <= xlen) bsize = bam::rd_u16(p + 12 + x + 4);
        x += 4 + slen;
    }
    if (bsize < 0) { *why = "gzip member without the BC extra field (plain gzip, not BGZF)"; return -1; }
    const int64_t total = bsize + 1;
    if (total < 12 + xlen + 8) { *why = "BSIZE smaller than the block's header and footer"; return -1; }
    if (left < total) return 1;
    b.off = at;
    b.bytes = (int32_t)total;
    b.cdata = at + 12 + xlen;
    b.clen = (int32_t)(total - 12 - xlen - 8);
    b.crc = bam::rd_u32(p + total - 8);
    b.isize = bam::rd_u32(p + total - 4);
    if (b.isize > 65536) { *why = "ISIZE above 65536"; return -1; }
    return 0;
}

// every complete block of data[0, n) (base = file offset of data[0]); returns the end of the last one, -1 on a framing error
static int64_t frame_blocks(const uint8_t *data, int64_t n, int64_t base, std::vector<BgzfBlock> &out, bool need_all)
{
    int64_t at = 0;
    while (at < n) {
        BgzfBlock b;
        const char *why = "";
        const int rc = frame_block(data, n, at, b, &why);
        if (rc < 0) return fail(ADVNTR_ERR_DATA, "BGZF: %s at file offset %lld", why, (long long)(base + at)), -1;
        if (rc > 0) {
            if (need_all) return fail(ADVNTR_ERR_DATA, "BGZF: truncated block at file offset %lld", (long long)(base + at)), -1;
            break;
        }
        b.off += base;
        b.cdata += base;
        out.push_back(b);
        at += b.bytes;
    }
    return at;
}

static const char *inflate_status_text(int s)
{
    switch (s) {
    case bgzf::INF_BAD_BLOCK_TYPE: return "invalid DEFLATE block type";
    case bgzf::INF_STORED_LEN: return "stored block length check failed";
    case bgzf::INF_TRUNCATED: return "DEFLATE stream ends early";
    case bgzf::INF_BAD_LENGTHS: return "invalid Huffman code lengths";
    case bgzf::INF_BAD_SYMBOL: return "invalid Huffman code";
    case bgzf::INF_DISTANCE: return "distance too far back";
    case bgzf::INF_OVERFLOW: return "more output than ISIZE";
    case bgzf::INF_ISIZE: return "less output than ISIZE";
    case bgzf::INF_CRC: return "CRC32 mismatch";
    default: return "unknown inflate status";
    }
}

// host inflate of one framed block (header parsing)
static int inflate_host(const uint8_t *file_data, int64_t file_base, const BgzfBlock &b, std::vector<uint8_t> &out)
{
    static thread_local bgzf::Tables T;
    const size_t at = out.size();
    out.resize(at + b.isize);
    bgzf::HostWave w;
    bgzf::fill_crc_table(T, w);
    uint32_t got = 0;
    int rc = bgzf::inflate_raw(file_data + (b.cdata - file_base), (uint32_t)b.clen, out.data() + at, b.isize, &got, T, w);
    if (rc == 0 && got != b.isize) rc = bgzf::INF_ISIZE;
    if (rc == 0 && bgzf::crc32_bytes(T.crc, out.data() + at, got) != b.crc) rc = bgzf::INF_CRC;
    if (rc) return fail(ADVNTR_ERR_DATA, "BGZF block at file offset %lld: %s", (long long)b.off, inflate_status_text(rc));
    return ADVNTR_OK;
}

struct BamHeader {
    std::vector<std::string> names;
    std::vector<int32_t> lengths;
    int64_t bytes = 0;
};

// inflate blocks from the start of the file on the host until the whole binary header is there
static int read_bam_header(const char *path, BamHeader &H)
{
    FILE *f = fopen(path, "rb");
    if (!f) return fail(ADVNTR_ERR_ARG, "cannot open %s", path);
    std::vector<uint8_t> raw, text;
    int64_t raw_base = 0;
    auto need = [&](int64_t bytes) -> int {       // inflate until `text` holds `bytes`
        while ((int64_t)text.size() < bytes) {
            std::vector<BgzfBlock> blocks;
            int64_t end = 0;
            for (;;) {
                end = frame_blocks(raw.data(), (int64_t)raw.size(), raw_base, blocks, false);
                if (end < 0) return ADVNTR_ERR_DATA;
                if (!blocks.empty()) break;
                uint8_t buf[1 << 16];
                const size_t got = fread(buf, 1, sizeof buf, f);
                if (got == 0) return fail(ADVNTR_ERR_DATA, "%s: the file ends inside the BAM header", path);
                raw.insert(raw.end(), buf, buf + got);
            }
            for (const BgzfBlock &b : blocks) {
                const int rc = inflate_host(raw.data(), raw_base, b, text);
                if (rc) return rc;
            }
            raw.erase(raw.begin(), raw.begin() + end);
            raw_base += end;
        }
        return ADVNTR_OK;
    };
    int rc = need(8);
    if (!rc && memcmp(text.data(), "BAM\1", 4) != 0) rc = fail(ADVNTR_ERR_DATA, "%s: no BAM magic", path);
    int64_t at = 0;
    if (!rc) {
        const int32_t l_text = bam::rd_i32(text.data() + 4);
        if (l_text < 0) rc = fail(ADVNTR_ERR_DATA, "%s: negative l_text", path);
        at = 8 + (int64_t)l_text;
        if (!rc) rc = need(at + 4);
    }
    if (!rc) {
        const int32_t n_ref = bam::rd_i32(text.data() + at);
        at += 4;
        if (n_ref < 0) rc = fail(ADVNTR_ERR_DATA, "%s: negative n_ref", path);
        for (int32_t r = 0; !rc && r < n_ref; ++r) {
            if ((rc = need(at + 4))) break;
            const int32_t l_name = bam::rd_i32(text.data() + at);
            if (l_name < 1) { rc = fail(ADVNTR_ERR_DATA, "%s: bad l_name of reference %d", path, r); break; }
            if ((rc = need(at + 4 + l_name + 4))) break;
            H.names.emplace_back((const char *)text.data() + at + 4, strnlen((const char *)text.data() + at + 4, l_name));
            H.lengths.push_back(bam::rd_i32(text.data() + at + 4 + l_name));
            at += 4 + l_name + 4;
        }
    }
    fclose(f);
    H.bytes = at;
    return rc;
}

double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

template <class T> struct DevBuf {       // a grow-only device buffer
    T *p = nullptr;
    size_t cap = 0;
    int ensure(size_t n)
    {
        if (n <= cap) return ADVNTR_OK;
        if (p) HIP_TRY(hipFree(p));
        p = nullptr;
        cap = 0;
        HIP_TRY(hipMalloc((void **)&p, std::max<size_t>(n, 1) * sizeof(T)));
        cap = n;
        return ADVNTR_OK;
    }
    ~DevBuf() { if (p) (void)hipFree(p); }
};

// the covered bases per window of an ADVNTR_BAM_COVERAGE pass (coverage_windows.h), resident on the device: reference r has
// n_windows[r] = length / 100 full windows at slots base[r] .. base[r] + n_windows[r] of diff (one more slot: the sink).  diff
// holds the difference arrays during the pass and every window's bp after the scan; zbits = the zero-length presence bits.
struct BamCoverage {
    bool on = false;
    std::vector<int64_t> base, n_windows;
    int64_t slots = 0;
    DevBuf<int64_t> d_base, d_n_windows, d_diff, d_tile;
    DevBuf<unsigned int> d_zbits;
    double stats[ADVNTR_BAM_COVERAGE_STATS] = {0};
};

}  // namespace

struct advntr_bam_kept {
    std::vector<int32_t> fields;
    std::vector<uint8_t> text;
    std::vector<int64_t> text_off{0};
    std::vector<int64_t> offsets;
    double stats[ADVNTR_BAM_STATS] = {0};
    BamCoverage cov;
};

extern "C" int advntr_bgzf_scan(const uint8_t *data, int64_t n_bytes, int64_t *block_off, int32_t *block_bytes, uint32_t *isize,
                                int64_t capacity, int64_t *n_blocks)
{
    if (!data || n_bytes < 0 || !n_blocks || capacity < 0) return fail(ADVNTR_ERR_ARG, "advntr_bgzf_scan: bad argument");
    std::vector<BgzfBlock> blocks;
    if (frame_blocks(data, n_bytes, 0, blocks, true) < 0) return ADVNTR_ERR_DATA;
    *n_blocks = (int64_t)blocks.size();
    for (int64_t i = 0; i < std::min<int64_t>(capacity, (int64_t)blocks.size()); ++i) {
        if (block_off) block_off[i] = blocks[i].off;
        if (block_bytes) block_bytes[i] = blocks[i].bytes;
        if (isize) isize[i] = blocks[i].isize;
    }
    return ADVNTR_OK;
}

extern "C" int advntr_bam_header(const char *path, char *names, int64_t names_capacity, int32_t *lengths, int32_t refs_capacity,
                                 int32_t *n_ref, int64_t *names_bytes, int64_t *header_bytes)
{
    if (!path || !n_ref || !names_bytes || !header_bytes) return fail(ADVNTR_ERR_ARG, "advntr_bam_header: bad argument");
    BamHeader H;
    const int rc = read_bam_header(path, H);
    if (rc) return rc;
    int64_t nb = 0;
    for (const std::string &s : H.names) nb += (int64_t)s.size() + 1;
    *n_ref = (int32_t)H.names.size();
    *names_bytes = nb;
    *header_bytes = H.bytes;
    if (names && names_capacity >= nb) {
        int64_t at = 0;
        for (const std::string &s : H.names) { memcpy(names + at, s.c_str(), s.size() + 1); at += (int64_t)s.size() + 1; }
    }
    if (lengths && refs_capacity >= *n_ref) std::copy(H.lengths.begin(), H.lengths.end(), lengths);
    return ADVNTR_OK;
}

extern "C" int advntr_bam_walk_host(const uint8_t *buf, int64_t n_bytes, int64_t start, int64_t *offsets, int64_t capacity,
                                    int64_t *n_records, int64_t *end)
{
    if (!buf || n_bytes < 0 || start < 0 || !n_records || !end) return fail(ADVNTR_ERR_ARG, "advntr_bam_walk_host: bad argument");
    int bad = 0;
    *end = bam::walk(buf, n_bytes, start, n_bytes, offsets, offsets ? capacity : 0, n_records, &bad);
    if (bad) return fail(ADVNTR_ERR_DATA, "BAM: block_size below %d at uncompressed offset %lld", bam::MIN_RECORD, (long long)*end);
    return ADVNTR_OK;
}

extern "C" int advntr_bam_decode_host(const uint8_t *buf, int64_t n_bytes, const int64_t *offsets, int64_t n_records,
                                      int32_t *fields, uint8_t *text, int64_t text_capacity, int64_t *text_off)
{
    if (!buf || n_records < 0 || (n_records && !offsets) || !text_off) return fail(ADVNTR_ERR_ARG, "advntr_bam_decode_host: bad argument");
    std::vector<bam::Record> recs((size_t)n_records);
    text_off[0] = 0;
    for (int64_t i = 0; i < n_records; ++i) {
        const int64_t o = offsets[i];
        if (o < 0 || o + 4 > n_bytes || o + 4 + (int64_t)bam::rd_i32(buf + o) > n_bytes || bam::rd_i32(buf + o) < bam::MIN_RECORD ||
            !bam::parse(buf, o, recs[i]))
            return fail(ADVNTR_ERR_DATA, "BAM: malformed record at uncompressed offset %lld", (long long)o);
        text_off[i + 1] = text_off[i] + bam::text_bytes(buf, recs[i]);
    }
    if (!fields || !text || text_capacity < text_off[n_records]) return ADVNTR_OK;
    for (int64_t i = 0; i < n_records; ++i) bam::decode(buf, recs[i], fields + bam::FIELDS * i, text + text_off[i]);
    return ADVNTR_OK;
}

namespace {

// device inflate of framed blocks whose compressed bytes are in d_comp at (cdata - comp_base); output at out_off
struct InflateLaunch {
    DevBuf<int64_t> cdata_off, out_off;
    DevBuf<int32_t> clen, status;
    DevBuf<uint32_t> isize, crc;
    std::vector<int64_t> h_cdata, h_out;
    std::vector<int32_t> h_clen, h_status;
    std::vector<uint32_t> h_isize, h_crc;

    // queue the launch; out_base = output offset of the first block
    int launch(const std::vector<BgzfBlock> &blocks, int64_t comp_base, const uint8_t *d_comp, int64_t out_base, uint8_t *d_out,
               hipStream_t s)
    {
        const size_t n = blocks.size();
        h_cdata.resize(n); h_out.resize(n); h_clen.resize(n); h_isize.resize(n); h_crc.resize(n);
        int64_t o = out_base;
        for (size_t i = 0; i < n; ++i) {
            h_cdata[i] = blocks[i].cdata - comp_base;
            h_clen[i] = blocks[i].clen;
            h_isize[i] = blocks[i].isize;
            h_crc[i] = blocks[i].crc;
            h_out[i] = o;
            o += blocks[i].isize;
        }
        int rc;
        if ((rc = cdata_off.ensure(n)) || (rc = out_off.ensure(n)) || (rc = clen.ensure(n)) || (rc = status.ensure(n)) ||
            (rc = isize.ensure(n)) || (rc = crc.ensure(n)))
            return rc;
        if (!n) return ADVNTR_OK;
        HIP_TRY(hipMemcpyAsync(cdata_off.p, h_cdata.data(), n * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(out_off.p, h_out.data(), n * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(clen.p, h_clen.data(), n * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(isize.p, h_isize.data(), n * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(crc.p, h_crc.data(), n * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(bgzf::inflate_blocks_kernel, dim3((unsigned)n), dim3(64), 0, s, d_comp, cdata_off.p, clen.p, isize.p,
                           crc.p, out_off.p, d_out, status.p, (int32_t)n);
        HIP_TRY(hipGetLastError());
        return ADVNTR_OK;
    }
    // after the stream is synchronised: the first failing block, by file offset
    int check(const std::vector<BgzfBlock> &blocks, hipStream_t s)
    {
        const size_t n = blocks.size();
        if (!n) return ADVNTR_OK;
        h_status.resize(n);
        HIP_TRY(hipMemcpyAsync(h_status.data(), status.p, n * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (size_t i = 0; i < n; ++i)
            if (h_status[i])
                return fail(ADVNTR_ERR_DATA, "BGZF block at file offset %lld: %s", (long long)blocks[i].off,
                            inflate_status_text(h_status[i]));
        return ADVNTR_OK;
    }
};

}  // namespace

extern "C" int advntr_bgzf_inflate(const uint8_t *data, int64_t n_bytes, uint8_t *out, int64_t out_capacity, int64_t *out_len)
{
    if (!data || n_bytes < 0 || !out_len || out_capacity < 0) return fail(ADVNTR_ERR_ARG, "advntr_bgzf_inflate: bad argument");
    if (advntr_device_count() <= 0) return fail(ADVNTR_ERR_DEVICE, "advntr_bgzf_inflate: no HIP device visible (no CPU fallback)");
    std::vector<BgzfBlock> blocks;
    if (frame_blocks(data, n_bytes, 0, blocks, true) < 0) return ADVNTR_ERR_DATA;
    int64_t total = 0;
    for (const BgzfBlock &b : blocks) total += b.isize;
    *out_len = total;
    if (!out || out_capacity < total) return fail(ADVNTR_ERR_ARG, "advntr_bgzf_inflate: output needs %lld bytes", (long long)total);
    (void)current_device();
    hipStream_t s = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    DevBuf<uint8_t> d_comp, d_out;
    InflateLaunch L;
    int rc = d_comp.ensure((size_t)n_bytes);
    if (!rc) rc = d_out.ensure((size_t)total);
    if (!rc && n_bytes) {
        const hipError_t e = hipMemcpyAsync(d_comp.p, data, (size_t)n_bytes, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) rc = fail(ADVNTR_ERR_DEVICE, "upload: %s", hipGetErrorString(e));
    }
    if (!rc) rc = L.launch(blocks, 0, d_comp.p, 0, d_out.p, s);
    if (!rc) rc = L.check(blocks, s);
    if (!rc && total) {
        const hipError_t e = hipMemcpyAsync(out, d_out.p, (size_t)total, hipMemcpyDeviceToHost, s);
        if (e != hipSuccess || hipStreamSynchronize(s) != hipSuccess) rc = fail(ADVNTR_ERR_DEVICE, "download failed");
    }
    (void)hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
    return rc;
}

namespace {

// one streaming pass: see advntr_bam_select in include/advntr_hip.h
struct BamScan {
    FILE *f = nullptr;
    const char *path = "";
    int64_t chunk = 0, file_at = 0;     // compressed bytes per chunk; file offset of pinned[slot][0]
    uint8_t *pinned[2] = {nullptr, nullptr};
    int64_t pinned_len[2] = {0, 0};     // bytes read into the slot (complete blocks + the partial tail)
    std::vector<BgzfBlock> blocks[2];
    int64_t blocks_end[2] = {0, 0};     // bytes of the slot's complete blocks
    bool eof = false;
    DevBuf<uint8_t> d_comp[2], d_out[2];
    hipStream_t s_copy = nullptr, s_run = nullptr;
    hipEvent_t uploaded[2] = {nullptr, nullptr}, up_t0[2] = {nullptr, nullptr}, k_t0 = nullptr, k_t1 = nullptr;
    advntr_bam_kept *K = nullptr;

    ~BamScan()
    {
        if (s_copy) (void)hipStreamSynchronize(s_copy);
        if (s_run) (void)hipStreamSynchronize(s_run);
        for (int i = 0; i < 2; ++i) {
            if (pinned[i]) (void)hipHostFree(pinned[i]);
            if (uploaded[i]) (void)hipEventDestroy(uploaded[i]);
            if (up_t0[i]) (void)hipEventDestroy(up_t0[i]);
        }
        if (k_t0) (void)hipEventDestroy(k_t0);
        if (k_t1) (void)hipEventDestroy(k_t1);
        if (s_copy) (void)hipStreamDestroy(s_copy);
        if (s_run) (void)hipStreamDestroy(s_run);
        if (f) fclose(f);
    }

    // read the next chunk into pinned[slot] (after the partial block left at the end of the other slot), frame it, and
    // queue its upload on the copy stream.  Returns ADVNTR_OK; blocks[slot] is empty at the end of the file.
    int prepare(int slot, int other, double *st)
    {
        auto t0 = std::chrono::steady_clock::now();
        int64_t keep = pinned_len[other] - blocks_end[other];
        if (keep > 0) memcpy(pinned[slot], pinned[other] + blocks_end[other], (size_t)keep);
        else keep = 0;
        const int64_t base = file_at + blocks_end[other];
        int64_t len = keep;
        const int64_t cap = chunk + 65536;
        while (!eof && len < cap) {
            const size_t got = fread(pinned[slot] + len, 1, (size_t)(cap - len), f);
            if (got == 0) eof = true;
            len += (int64_t)got;
        }
        st[6] += ms_since(t0);
        t0 = std::chrono::steady_clock::now();
        file_at = base;
        pinned_len[slot] = len;
        blocks[slot].clear();
        // frame whole blocks up to `chunk` bytes (at least one block)
        int64_t at = 0;
        while (at < len) {
            BgzfBlock b;
            const char *why = "";
            const int rc = frame_block(pinned[slot], len, at, b, &why);
            if (rc < 0) return fail(ADVNTR_ERR_DATA, "%s: BGZF: %s at file offset %lld", path, why, (long long)(base + at));
            if (rc > 0) {
                if (eof) return fail(ADVNTR_ERR_DATA, "%s: BGZF: truncated block at file offset %lld", path, (long long)(base + at));
                break;
            }
            if (at > 0 && at + b.bytes > chunk) break;
            b.off += base;
            b.cdata += base;
            blocks[slot].push_back(b);
            at += b.bytes;
        }
        blocks_end[slot] = at;
        st[7] += ms_since(t0);
        if (at) {
            int rc = d_comp[slot].ensure((size_t)at);
            if (rc) return rc;
            HIP_TRY(hipEventRecord(up_t0[slot], s_copy));
            HIP_TRY(hipMemcpyAsync(d_comp[slot].p, pinned[slot], (size_t)at, hipMemcpyHostToDevice, s_copy));
            HIP_TRY(hipEventRecord(uploaded[slot], s_copy));
        }
        return ADVNTR_OK;
    }
};

}  // namespace

namespace {

// windows per reference sorted by start (ties by end), with the running maximum of their ends; order[j] = input index of
// sorted window j
struct SortedWindows {
    std::vector<int64_t> start, end, maxend;
    std::vector<int32_t> order;
};

static int sort_windows(const char *who, int32_t n_ref, const int32_t *win_ptr, const int64_t *win_start, const int64_t *win_end,
                        SortedWindows &W)
{
    const int32_t n_win = n_ref ? win_ptr[n_ref] : 0;
    W.start.resize(n_win); W.end.resize(n_win); W.maxend.resize(n_win); W.order.resize(n_win);
    for (int32_t r = 0; r < n_ref; ++r) {
        if (win_ptr[r + 1] < win_ptr[r]) return fail(ADVNTR_ERR_ARG, "%s: win_ptr not monotone", who);
        std::vector<std::tuple<int64_t, int64_t, int32_t>> w;
        for (int32_t k = win_ptr[r]; k < win_ptr[r + 1]; ++k) w.emplace_back(win_start[k], win_end[k], k);
        std::sort(w.begin(), w.end());
        int64_t m = INT64_MIN;
        for (size_t k = 0; k < w.size(); ++k) {
            const size_t j = win_ptr[r] + k;
            W.start[j] = std::get<0>(w[k]);
            W.end[j] = std::get<1>(w[k]);
            W.maxend[j] = m = std::max(m, std::get<1>(w[k]));
            W.order[j] = std::get<2>(w[k]);
        }
    }
    return ADVNTR_OK;
}

// What a pass does with the complete records of one chunk while they are resident: d_buf[d_offs[i]] for i < n_rec, on stream
// s; records_before = records of the earlier chunks, at = uncompressed file offset of d_buf[0].
typedef std::function<int(const uint8_t *d_buf, const int64_t *d_offs, int64_t n_rec, int64_t records_before, int64_t at,
                          hipStream_t s)>
    ChunkFn;

// one streaming pass over the records of a BAM file (see advntr_bam_select in include/advntr_hip.h); stats st[0..15]
static int bam_stream(const char *who, const char *path, int32_t n_ref, int64_t chunk_bytes, bool keep_offsets,
                      std::vector<int64_t> &offsets, double *st, const ChunkFn &on_chunk)
{
    const auto t_all = std::chrono::steady_clock::now();
    BamHeader H;
    int rc = read_bam_header(path, H);
    if (rc) return rc;
    if ((int32_t)H.names.size() != n_ref)
        return fail(ADVNTR_ERR_ARG, "%s: %d window lists for %d references", who, n_ref, (int)H.names.size());
    BamScan S;
    S.path = path;
    S.chunk = chunk_bytes > 0 ? chunk_bytes : (int64_t)256 << 20;
    S.f = fopen(path, "rb");
    if (!S.f) return fail(ADVNTR_ERR_ARG, "cannot open %s", path);
    (void)current_device();
#define BAM_RC(expr)                                                                                                      \
    do {                                                                                                                  \
        if ((rc = (expr)) != ADVNTR_OK) return rc;                                                                        \
    } while (0)
    HIP_TRY(hipStreamCreateWithFlags(&S.s_copy, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&S.s_run, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(hipHostMalloc((void **)&S.pinned[i], (size_t)(S.chunk + 65536), hipHostMallocDefault));
        HIP_TRY(hipEventCreate(&S.uploaded[i]));
        HIP_TRY(hipEventCreate(&S.up_t0[i]));
    }
    HIP_TRY(hipEventCreate(&S.k_t0));
    HIP_TRY(hipEventCreate(&S.k_t1));
    DevBuf<int32_t> d_count;
    DevBuf<int64_t> d_start, d_stop, d_end, d_base, d_offs;
    InflateLaunch L;
    int64_t uncompressed_before = 0;    // uncompressed bytes of the blocks before the current chunk
    int64_t records_before = 0, carry = 0;
    std::vector<int64_t> h_start, h_stop, h_end, h_base, h_offs;
    std::vector<int32_t> h_count;
    std::vector<uint8_t> window;        // host copy of d_out[lo, lo + window.size()) for the fallback walk
    BAM_RC(S.prepare(0, 1, st));
    for (int slot = 0; !S.blocks[slot].empty(); slot ^= 1) {
        const std::vector<BgzfBlock> &B = S.blocks[slot];
        const int nb = (int)B.size();
        int64_t isum = 0;
        for (const BgzfBlock &b : B) isum += b.isize;
        const int64_t buflen = carry + isum;
        // carry bytes are already at the front of d_out[slot] (moved at the end of the previous chunk)
        BAM_RC(S.d_out[slot].ensure((size_t)std::max<int64_t>(buflen, 1)));
        uint8_t *d_buf = S.d_out[slot].p;
        HIP_TRY(hipStreamWaitEvent(S.s_run, S.uploaded[slot], 0));
        HIP_TRY(hipEventRecord(S.k_t0, S.s_run));
        BAM_RC(L.launch(B, S.blocks[slot].front().off, S.d_comp[slot].p, carry, d_buf, S.s_run));
        HIP_TRY(hipEventRecord(S.k_t1, S.s_run));
        // assumed record starts: the first byte of every block (the chunk's first: the carry, or the end of the header)
        const int64_t first = carry ? 0 : std::max<int64_t>(0, H.bytes - uncompressed_before);
        h_start.resize(nb); h_stop.resize(nb); h_end.resize(nb); h_count.resize(nb); h_base.resize(nb);
        int64_t o = carry;
        for (int b = 0; b < nb; ++b) {
            h_start[b] = b == 0 ? std::min(first, buflen) : std::max(o, std::min(first, buflen));
            h_stop[b] = o + B[b].isize;
            o += B[b].isize;
        }
        BAM_RC(d_start.ensure(nb)); BAM_RC(d_stop.ensure(nb)); BAM_RC(d_end.ensure(nb)); BAM_RC(d_count.ensure(nb));
        BAM_RC(d_base.ensure(nb));
        HIP_TRY(hipMemcpyAsync(d_start.p, h_start.data(), nb * 8, hipMemcpyHostToDevice, S.s_run));
        HIP_TRY(hipMemcpyAsync(d_stop.p, h_stop.data(), nb * 8, hipMemcpyHostToDevice, S.s_run));
        hipLaunchKernelGGL(bam::walk_blocks_kernel, dim3((nb + 255) / 256), dim3(256), 0, S.s_run, d_buf, buflen, d_start.p, d_stop.p,
                           nb, d_end.p, d_count.p, (const int64_t *)nullptr, (int64_t *)nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_end.data(), d_end.p, nb * 8, hipMemcpyDeviceToHost, S.s_run));
        HIP_TRY(hipMemcpyAsync(h_count.data(), d_count.p, nb * 4, hipMemcpyDeviceToHost, S.s_run));
        // the next chunk is read, framed and uploaded while this one's kernels run
        BAM_RC(S.prepare(slot ^ 1, slot, st));
        BAM_RC(L.check(B, S.s_run));         // synchronises s_run
        {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, S.k_t0, S.k_t1));
            st[9] += ms;
            HIP_TRY(hipEventSynchronize(S.uploaded[slot]));
            HIP_TRY(hipEventElapsedTime(&ms, S.up_t0[slot], S.uploaded[slot]));
            st[8] += ms;
        }
        const auto t_walk = std::chrono::steady_clock::now();
        // confirm the chain: block b's walk holds when it started where block b-1's ended; a failing stretch is walked here
        int64_t lo = 0;
        window.clear();
        auto fetch_window = [&](int64_t a, int64_t z) -> int {        // window covers [a, z)
            if (a >= lo && z <= lo + (int64_t)window.size()) return ADVNTR_OK;
            lo = a;
            const int64_t hi = std::min(buflen, std::max(z, a + ((int64_t)4 << 20)));
            window.resize((size_t)(hi - a));
            HIP_TRY(hipMemcpy(window.data(), d_buf + a, (size_t)(hi - a), hipMemcpyDeviceToHost));
            return ADVNTR_OK;
        };
        int64_t s = h_start[0], total = 0;
        bool tail = false;
        for (int b = 0; b < nb; ++b) {
            if (tail) {
                h_start[b] = h_stop[b];
                h_count[b] = 0;
            } else if (s == h_start[b] && h_end[b] >= 0) {
                s = h_end[b];
            } else {
                const auto t_fb = std::chrono::steady_clock::now();
                st[11] += 1;
                BAM_RC(fetch_window(s, std::min(buflen, std::max(s, h_stop[b]) + 4)));
                int64_t p = s, c = 0;
                while (p < h_stop[b] && p + 4 <= buflen) {
                    const int32_t bs = bam::rd_i32(window.data() + (p - lo));
                    if (bs < bam::MIN_RECORD)
                        return fail(ADVNTR_ERR_DATA, "%s: BAM record with block_size %d at uncompressed offset %lld", path, bs,
                                    (long long)(uncompressed_before - carry + p));
                    if (p + 4 + (int64_t)bs > buflen) break;
                    ++c;
                    p += 4 + (int64_t)bs;
                    if (p < h_stop[b]) BAM_RC(fetch_window(p, std::min(buflen, h_stop[b] + 4)));
                }
                h_start[b] = s;
                h_count[b] = (int32_t)c;
                h_end[b] = p;
                s = p;
                st[12] += ms_since(t_fb);
            }
            if (!tail && s < h_stop[b]) tail = true;    // stopped at a record that does not fit: the rest is the carry
            h_base[b] = total;
            total += h_count[b];
        }
        const int64_t n_rec = total, carry_next = buflen - s;
        if (n_rec) {
            BAM_RC(d_offs.ensure(n_rec));
            HIP_TRY(hipMemcpyAsync(d_start.p, h_start.data(), nb * 8, hipMemcpyHostToDevice, S.s_run));
            HIP_TRY(hipMemcpyAsync(d_count.p, h_count.data(), nb * 4, hipMemcpyHostToDevice, S.s_run));
            HIP_TRY(hipMemcpyAsync(d_base.p, h_base.data(), nb * 8, hipMemcpyHostToDevice, S.s_run));
            hipLaunchKernelGGL(bam::walk_blocks_kernel, dim3((nb + 255) / 256), dim3(256), 0, S.s_run, d_buf, buflen, d_start.p,
                               d_stop.p, nb, d_end.p, d_count.p, d_base.p, d_offs.p);
            HIP_TRY(hipGetLastError());
            if (keep_offsets) {
                h_offs.resize(n_rec);
                HIP_TRY(hipMemcpyAsync(h_offs.data(), d_offs.p, n_rec * 8, hipMemcpyDeviceToHost, S.s_run));
                HIP_TRY(hipStreamSynchronize(S.s_run));
                for (int64_t i = 0; i < n_rec; ++i) offsets.push_back(uncompressed_before - carry + h_offs[i]);
            }
        }
        HIP_TRY(hipStreamSynchronize(S.s_run));
        st[10] += ms_since(t_walk);
        const auto t_sel = std::chrono::steady_clock::now();
        if (n_rec) BAM_RC(on_chunk(d_buf, d_offs.p, n_rec, records_before, uncompressed_before - carry, S.s_run));
        st[13] += ms_since(t_sel);
        // the bytes of the record that did not fit go to the front of the next chunk's output
        const std::vector<BgzfBlock> &N = S.blocks[slot ^ 1];
        if (N.empty() && carry_next > 0)
            return fail(ADVNTR_ERR_DATA, "%s: the file ends inside a BAM record (uncompressed offset %lld)", path,
                        (long long)(uncompressed_before - carry + s));
        int64_t next_isum = 0;
        for (const BgzfBlock &b : N) next_isum += b.isize;
        BAM_RC(S.d_out[slot ^ 1].ensure((size_t)std::max<int64_t>(1, carry_next + next_isum)));
        if (carry_next)
            HIP_TRY(hipMemcpyAsync(S.d_out[slot ^ 1].p, d_buf + s, (size_t)carry_next, hipMemcpyDeviceToDevice, S.s_run));
        st[0] += nb;
        st[1] += (double)(B.back().off + B.back().bytes - B.front().off);
        st[2] += (double)isum;
        st[3] += (double)n_rec;
        st[5] += 1;
        records_before += n_rec;
        uncompressed_before += isum;
        carry = carry_next;
    }
    HIP_TRY(hipStreamSynchronize(S.s_run));
    if (H.bytes > uncompressed_before) return fail(ADVNTR_ERR_DATA, "%s: the file ends inside the BAM header", path);
    st[14] = ms_since(t_all);
#undef BAM_RC
    return ADVNTR_OK;
}

// the malformed-record error of a chunk: bad = index of the first record whose parts overrun it
static int bad_record(const char *path, const int64_t *d_offs, unsigned long long bad, int64_t at)
{
    int64_t o = 0;
    HIP_TRY(hipMemcpy(&o, d_offs + bad, 8, hipMemcpyDeviceToHost));
    return fail(ADVNTR_ERR_DATA, "%s: malformed BAM record at uncompressed offset %lld", path, (long long)(at + o));
}

// decode records kept_idx[k] (file order) whole into K (fields / text / text_off), kept_bytes[k] = their text bytes
struct WholeDecode {
    DevBuf<int64_t> d_kidx, d_toff;
    DevBuf<int32_t> d_fields;
    DevBuf<uint8_t> d_text;
    std::vector<int64_t> h_kidx, h_toff;

    int run(const uint8_t *d_buf, const int64_t *d_offs, std::vector<std::pair<int64_t, int64_t>> &kept, advntr_bam_kept *K,
            hipStream_t s)
    {
        const int64_t nk = (int64_t)kept.size();
        if (!nk) return ADVNTR_OK;
        std::sort(kept.begin(), kept.end());
        h_kidx.resize(nk);
        h_toff.resize(nk + 1);
        h_toff[0] = 0;
        for (int64_t i = 0; i < nk; ++i) {
            h_kidx[i] = kept[i].first;
            h_toff[i + 1] = h_toff[i] + kept[i].second;
        }
        int rc;
        if ((rc = d_kidx.ensure(nk)) || (rc = d_toff.ensure(nk + 1)) || (rc = d_fields.ensure(nk * bam::FIELDS)) ||
            (rc = d_text.ensure((size_t)std::max<int64_t>(1, h_toff[nk]))))
            return rc;
        HIP_TRY(hipMemcpyAsync(d_kidx.p, h_kidx.data(), nk * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_toff.p, h_toff.data(), (nk + 1) * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(bam::decode_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, s, d_buf, d_offs, d_kidx.p,
                           d_toff.p, nk, d_fields.p, d_text.p);
        HIP_TRY(hipGetLastError());
        const size_t f0 = K->fields.size(), t0 = K->text.size();
        K->fields.resize(f0 + nk * bam::FIELDS);
        K->text.resize(t0 + h_toff[nk]);
        HIP_TRY(hipMemcpyAsync(K->fields.data() + f0, d_fields.p, nk * bam::FIELDS * 4, hipMemcpyDeviceToHost, s));
        if (h_toff[nk]) HIP_TRY(hipMemcpyAsync(K->text.data() + t0, d_text.p, h_toff[nk], hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (int64_t i = 0; i < nk; ++i) K->text_off.push_back((int64_t)t0 + h_toff[i + 1]);
        K->stats[4] += (double)nk;
        return ADVNTR_OK;
    }
};

}  // namespace

namespace {

// an ADVNTR_BAM_COVERAGE pass: the window layout from the header's lengths, the zeroed arrays, the events of the timings
static int coverage_setup(const char *who, const char *path, int32_t n_ref, BamCoverage &C, hipEvent_t *ev)
{
    BamHeader H;
    int rc = read_bam_header(path, H);
    if (rc) return rc;
    if ((int32_t)H.names.size() != n_ref) return fail(ADVNTR_ERR_ARG, "%s: %d window lists for %d references", who, n_ref, (int)H.names.size());
    C.base.assign(n_ref, -1);
    C.n_windows.assign(n_ref, 0);
    C.slots = 0;
    for (int32_t r = 0; r < n_ref; ++r) {
        C.n_windows[r] = std::max<int64_t>(0, H.lengths[r]) / cov::WINDOW;
        if (!C.n_windows[r]) continue;
        C.base[r] = C.slots;
        C.slots += C.n_windows[r] + 1;
    }
    const int64_t words = (C.slots + 31) / 32;
    (void)current_device();
    for (int i = 0; i < 2; ++i) HIP_TRY(hipEventCreate(&ev[i]));
    if ((rc = C.d_base.ensure(std::max(n_ref, 1))) || (rc = C.d_n_windows.ensure(std::max(n_ref, 1))) ||
        (rc = C.d_diff.ensure(std::max<int64_t>(1, C.slots))) || (rc = C.d_zbits.ensure(std::max<int64_t>(1, words))))
        return rc;
    if (n_ref) {
        HIP_TRY(hipMemcpy(C.d_base.p, C.base.data(), n_ref * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(C.d_n_windows.p, C.n_windows.data(), n_ref * 8, hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemset(C.d_diff.p, 0, std::max<int64_t>(1, C.slots) * 8));
    HIP_TRY(hipMemset(C.d_zbits.p, 0, std::max<int64_t>(1, words) * 4));
    HIP_TRY(hipStreamSynchronize(nullptr));         // the pass runs on non-blocking streams: the zeros land first
    for (int32_t r = 0; r < n_ref; ++r) C.stats[5] += (double)C.n_windows[r];
    C.on = true;
    return ADVNTR_OK;
}

// after the last chunk: one inclusive scan over all references' slots turns the difference arrays into bp per window
static int coverage_scan(BamCoverage &C, hipEvent_t *ev)
{
    if (!C.slots) return ADVNTR_OK;
    const int64_t tiles = (C.slots + cov::SCAN_TILE - 1) / cov::SCAN_TILE;
    int rc = C.d_tile.ensure(tiles);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(ev[0], nullptr));
    hipLaunchKernelGGL(cov::tile_sums_kernel, dim3((unsigned)tiles), dim3(cov::SCAN_THREADS), 0, nullptr, C.d_diff.p, C.slots, C.d_tile.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(cov::tile_prefix_kernel, dim3(1), dim3(cov::SCAN_THREADS), 0, nullptr, C.d_tile.p, tiles);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(cov::tile_scan_kernel, dim3((unsigned)tiles), dim3(cov::SCAN_THREADS), 0, nullptr, C.d_diff.p, C.slots, C.d_tile.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[1], nullptr));
    HIP_TRY(hipEventSynchronize(ev[1]));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    C.stats[1] += ms;
    return ADVNTR_OK;
}

}  // namespace

extern "C" advntr_bam_kept *advntr_bam_select(const char *path, int32_t n_ref, const int32_t *win_ptr, const int64_t *win_start,
                                              const int64_t *win_end, int64_t chunk_bytes, uint32_t flags)
{
    if (!path || n_ref < 0 || (n_ref && !win_ptr)) return fail(ADVNTR_ERR_ARG, "advntr_bam_select: bad argument"), nullptr;
    const int32_t n_win = n_ref ? win_ptr[n_ref] : 0;
    if (n_win < 0 || (n_win && (!win_start || !win_end))) return fail(ADVNTR_ERR_ARG, "advntr_bam_select: bad windows"), nullptr;
    if (advntr_device_count() <= 0) return fail(ADVNTR_ERR_DEVICE, "advntr_bam_select: no HIP device visible (no CPU fallback)"), nullptr;
    SortedWindows W;
    if (sort_windows("advntr_bam_select", n_ref, win_ptr, win_start, win_end, W)) return nullptr;
    std::unique_ptr<advntr_bam_kept> K(new advntr_bam_kept());
    DevBuf<int32_t> d_win_ptr;
    DevBuf<int64_t> d_ws, d_wmax, d_kidx, d_kbytes;
    DevBuf<unsigned long long> d_counters;
    WholeDecode D;
    if (d_win_ptr.ensure(n_ref + 1) || d_ws.ensure(n_win) || d_wmax.ensure(n_win) || d_counters.ensure(2)) return nullptr;
    std::vector<int32_t> wp(win_ptr, win_ptr + n_ref + 1);
    if (!n_ref) wp.assign(1, 0);
    std::vector<int64_t> h_kidx, h_kbytes;
    std::vector<std::pair<int64_t, int64_t>> kept;
    BamCoverage &C = K->cov;
    hipEvent_t ce[2] = {nullptr, nullptr};
    struct Events {
        hipEvent_t *e;
        ~Events() { for (int i = 0; i < 2; ++i) if (e[i]) (void)hipEventDestroy(e[i]); }
    } events_guard{ce};
    const ChunkFn select = [&](const uint8_t *d_buf, const int64_t *d_offs, int64_t n_rec, int64_t records_before, int64_t at,
                               hipStream_t s) -> int {
        int rc;
        if ((rc = d_kidx.ensure(n_rec)) || (rc = d_kbytes.ensure(n_rec))) return rc;
        if (C.on) {         // the window accumulation of the same resident records, ahead of the selection on the same stream
            HIP_TRY(hipEventRecord(ce[0], s));
            hipLaunchKernelGGL(cov::accumulate_kernel, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, s, d_buf, d_offs, n_rec,
                               n_ref, C.d_base.p, C.d_n_windows.p, (unsigned long long *)C.d_diff.p, C.d_zbits.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(ce[1], s));
        }
        const unsigned long long init[2] = {0, ~0ull};
        HIP_TRY(hipMemcpyAsync(d_counters.p, init, sizeof init, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(bam::select_kernel, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, s, d_buf, d_offs, n_rec,
                           std::max<int64_t>(0, 5 - records_before), n_ref, d_win_ptr.p, d_ws.p, d_wmax.p, d_counters.p,
                           d_kidx.p, d_kbytes.p, n_rec, d_counters.p + 1);
        HIP_TRY(hipGetLastError());
        unsigned long long cnt[2];
        HIP_TRY(hipMemcpyAsync(cnt, d_counters.p, sizeof cnt, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (C.on) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, ce[0], ce[1]));
            C.stats[0] += ms;
        }
        if (cnt[1] != ~0ull) return bad_record(path, d_offs, cnt[1], at);
        const int64_t nk = (int64_t)cnt[0];
        if (!nk) return ADVNTR_OK;
        h_kidx.resize(nk); h_kbytes.resize(nk);
        HIP_TRY(hipMemcpy(h_kidx.data(), d_kidx.p, nk * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(h_kbytes.data(), d_kbytes.p, nk * 8, hipMemcpyDeviceToHost));
        kept.resize(nk);
        for (int64_t i = 0; i < nk; ++i) kept[i] = {h_kidx[i], h_kbytes[i]};
        return D.run(d_buf, d_offs, kept, K.get(), s);
    };
    (void)current_device();
    if (hipMemcpy(d_win_ptr.p, wp.data(), wp.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        (n_win && (hipMemcpy(d_ws.p, W.start.data(), n_win * 8, hipMemcpyHostToDevice) != hipSuccess ||
                   hipMemcpy(d_wmax.p, W.maxend.data(), n_win * 8, hipMemcpyHostToDevice) != hipSuccess)))
        return fail(ADVNTR_ERR_DEVICE, "advntr_bam_select: window upload failed"), nullptr;
    if ((flags & ADVNTR_BAM_COVERAGE) && coverage_setup("advntr_bam_select", path, n_ref, C, ce)) return nullptr;
    if (bam_stream("advntr_bam_select", path, n_ref, chunk_bytes, flags & ADVNTR_BAM_RECORD_OFFSETS, K->offsets, K->stats, select))
        return nullptr;
    if (C.on && coverage_scan(C, ce)) return nullptr;
    return K.release();
}

extern "C" int advntr_bam_kept_info(const advntr_bam_kept *K, int64_t *n_kept, int64_t *text_bytes, int64_t *n_offsets, double *stats)
{
    if (!K) return fail(ADVNTR_ERR_ARG, "advntr_bam_kept_info: null handle");
    if (n_kept) *n_kept = (int64_t)K->text_off.size() - 1;
    if (text_bytes) *text_bytes = (int64_t)K->text.size();
    if (n_offsets) *n_offsets = (int64_t)K->offsets.size();
    if (stats) std::copy(K->stats, K->stats + ADVNTR_BAM_STATS, stats);
    return ADVNTR_OK;
}

extern "C" int advntr_bam_kept_fetch(const advntr_bam_kept *K, int32_t *fields, uint8_t *text, int64_t *text_off)
{
    if (!K) return fail(ADVNTR_ERR_ARG, "advntr_bam_kept_fetch: null handle");
    if (fields) std::copy(K->fields.begin(), K->fields.end(), fields);
    if (text) std::copy(K->text.begin(), K->text.end(), text);
    if (text_off) std::copy(K->text_off.begin(), K->text_off.end(), text_off);
    return ADVNTR_OK;
}

extern "C" int advntr_bam_kept_offsets(const advntr_bam_kept *K, int64_t *offsets)
{
    if (!K) return fail(ADVNTR_ERR_ARG, "advntr_bam_kept_offsets: null handle");
    if (offsets) std::copy(K->offsets.begin(), K->offsets.end(), offsets);
    return ADVNTR_OK;
}

extern "C" void advntr_bam_kept_destroy(advntr_bam_kept *K) { delete K; }

struct advntr_bam_spans {
    advntr_bam_kept unmapped;                   // unmapped records, decoded whole (fields / text / text_off)
    std::vector<int64_t> pairs;                 // ADVNTR_BAM_SPAN_FIELDS per (window, record) pair
    std::vector<uint8_t> text;                  // per pair: name | trimmed piece (empty unless spanning)
    std::vector<int64_t> text_off{0};
    double stats[ADVNTR_BAM_SPAN_STATS] = {0};
};

namespace {

const int SPAN_FIELDS = ADVNTR_BAM_SPAN_FIELDS;

static void put_pair(int64_t *o, int64_t window, int64_t locus, int64_t record, const bam::Span &s, int64_t name_len)
{
    o[0] = window; o[1] = locus; o[2] = record; o[3] = s.status; o[4] = s.rs; o[5] = s.end;
    o[6] = s.left; o[7] = s.tr; o[8] = s.right; o[9] = name_len;
}

static int cg_error(const char *where, const std::string &name, long long at)
{
    return fail(ADVNTR_ERR_DATA, "%sBAM record '%s' at uncompressed offset %lld: its CIGAR is kept in the CG tag (<l_seq>S<ref_len>N "
                "placeholder), which is not decoded", where, name.c_str(), at);
}

}  // namespace

extern "C" int advntr_bam_span_host(const uint8_t *buf, int64_t n_bytes, const int64_t *offsets, const int64_t *win_start,
                                    const int64_t *win_end, int64_t n, int32_t flank, int32_t min_flank, int64_t *pairs,
                                    uint8_t *text, int64_t text_capacity, int64_t *text_off)
{
    if (!buf || n < 0 || (n && (!offsets || !win_start || !win_end)) || !text_off || flank < 0 || min_flank < 0)
        return fail(ADVNTR_ERR_ARG, "advntr_bam_span_host: bad argument");
    std::vector<bam::Record> recs((size_t)n);
    std::vector<bam::Span> spans((size_t)n);
    text_off[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t o = offsets[i];
        if (o < 0 || o + 4 > n_bytes || o + 4 + (int64_t)bam::rd_i32(buf + o) > n_bytes || bam::rd_i32(buf + o) < bam::MIN_RECORD ||
            !bam::parse(buf, o, recs[i]))
            return fail(ADVNTR_ERR_DATA, "BAM: malformed record at uncompressed offset %lld", (long long)o);
        spans[i] = bam::span_host(buf, recs[i], win_start[i], win_end[i], flank, min_flank);
        if (spans[i].status == bam::SPAN_CG_TAG)
            return cg_error("", std::string((const char *)buf + recs[i].name_at, recs[i].l_name - 1), (long long)o);
        text_off[i + 1] = text_off[i] + (spans[i].status == bam::SPAN_OK ? recs[i].l_name - 1 + spans[i].end - spans[i].rs : 0);
    }
    if (pairs)
        for (int64_t i = 0; i < n; ++i) put_pair(pairs + SPAN_FIELDS * i, i, -1, i, spans[i], recs[i].l_name - 1);
    if (!text || text_capacity < text_off[n]) return ADVNTR_OK;
    for (int64_t i = 0; i < n; ++i) {
        if (spans[i].status != bam::SPAN_OK) continue;
        uint8_t *dst = text + text_off[i];
        const bam::Record &r = recs[i];
        for (int32_t k = 0; k < r.l_name - 1; ++k) *dst++ = buf[r.name_at + k];
        for (int64_t k = spans[i].rs; k < spans[i].end; ++k) bam::decode_piece_base(buf, r, k, dst++);
    }
    return ADVNTR_OK;
}

extern "C" advntr_bam_spans *advntr_bam_select_spans(const char *path, int32_t n_ref, const int32_t *win_ptr, const int64_t *win_start,
                                                     const int64_t *win_end, const int64_t *win_locus, int32_t flank,
                                                     int32_t min_flank, int64_t chunk_bytes, uint32_t flags)
{
    const char *who = "advntr_bam_select_spans";
    if (!path || n_ref < 0 || (n_ref && !win_ptr) || flank < 0 || min_flank < 0) return fail(ADVNTR_ERR_ARG, "%s: bad argument", who), nullptr;
    const int32_t n_win = n_ref ? win_ptr[n_ref] : 0;
    if (n_win < 0 || (n_win && (!win_start || !win_end || !win_locus))) return fail(ADVNTR_ERR_ARG, "%s: bad windows", who), nullptr;
    if (advntr_device_count() <= 0) return fail(ADVNTR_ERR_DEVICE, "%s: no HIP device visible (no CPU fallback)", who), nullptr;
    SortedWindows W;
    if (sort_windows(who, n_ref, win_ptr, win_start, win_end, W)) return nullptr;
    std::unique_ptr<advntr_bam_spans> P(new advntr_bam_spans());
    double *st = P->stats;
    DevBuf<int32_t> d_win_ptr, d_pwin;
    DevBuf<int64_t> d_ws, d_we, d_wmax, d_kidx, d_kbytes, d_prec, d_out, d_trec, d_trs, d_tend, d_ttoff;
    DevBuf<unsigned long long> d_counters;
    DevBuf<uint8_t> d_text;
    WholeDecode D;
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    struct Events {
        hipEvent_t *e;
        ~Events() { for (int i = 0; i < 4; ++i) if (e[i]) (void)hipEventDestroy(e[i]); }
    } events_guard{e};
    if (d_win_ptr.ensure(n_ref + 1) || d_ws.ensure(n_win) || d_we.ensure(n_win) || d_wmax.ensure(n_win) || d_counters.ensure(4))
        return nullptr;
    std::vector<int32_t> wp(win_ptr, win_ptr + n_ref + 1);
    if (!n_ref) wp.assign(1, 0);
    int64_t pair_cap = 0;
    std::vector<int64_t> h_kidx, h_kbytes, h_prec, h_out, t_rec, t_rs, t_end, t_toff;
    std::vector<int32_t> h_pwin;
    std::vector<std::pair<int64_t, int64_t>> kept;
    std::vector<size_t> order;
    const ChunkFn spans = [&](const uint8_t *d_buf, const int64_t *d_offs, int64_t n_rec, int64_t records_before, int64_t at,
                              hipStream_t s) -> int {
        int rc;
        if ((rc = d_kidx.ensure(n_rec)) || (rc = d_kbytes.ensure(n_rec))) return rc;
        unsigned long long cnt[4];
        for (;;) {          // at most twice: a second launch when the pairs outgrew the buffers
            pair_cap = std::max<int64_t>(pair_cap, std::max<int64_t>(1024, 2 * n_rec));
            if ((rc = d_prec.ensure(pair_cap)) || (rc = d_pwin.ensure(pair_cap))) return rc;
            const unsigned long long init[4] = {0, 0, ~0ull, 0};
            HIP_TRY(hipMemcpyAsync(d_counters.p, init, sizeof init, hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(bam::span_select_kernel, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, s, d_buf, d_offs, n_rec,
                               n_ref, d_win_ptr.p, d_ws.p, d_we.p, d_wmax.p, d_counters.p, d_kidx.p, d_kbytes.p, n_rec, d_prec.p,
                               d_pwin.p, pair_cap);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(cnt, d_counters.p, sizeof cnt, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            if (cnt[2] != ~0ull) return bad_record(path, d_offs, cnt[2], at);
            if ((int64_t)cnt[1] <= pair_cap) break;
            pair_cap = (int64_t)cnt[1];
        }
        const int64_t np = (int64_t)cnt[1];
        st[26] += (double)cnt[3];
        if (np) {
            if ((rc = d_out.ensure(np * bam::SPAN_OUT))) return rc;
            HIP_TRY(hipEventRecord(e[0], s));
            hipLaunchKernelGGL(bam::span_kernel, dim3((unsigned)((np + 3) / 4)), dim3(256), 0, s, d_buf, d_offs, d_prec.p, d_pwin.p, np,
                               d_ws.p, d_we.p, (int64_t)flank, (int64_t)min_flank, d_out.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(e[1], s));
            h_prec.resize(np); h_pwin.resize(np); h_out.resize(np * bam::SPAN_OUT);
            HIP_TRY(hipMemcpyAsync(h_prec.data(), d_prec.p, np * 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(h_pwin.data(), d_pwin.p, np * 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(h_out.data(), d_out.p, np * bam::SPAN_OUT * 8, hipMemcpyDeviceToHost, s));
        }
        const int64_t nk = (int64_t)cnt[0];
        h_kidx.resize(nk); h_kbytes.resize(nk);
        if (nk) {
            HIP_TRY(hipMemcpyAsync(h_kidx.data(), d_kidx.p, nk * 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(h_kbytes.data(), d_kbytes.p, nk * 8, hipMemcpyDeviceToHost, s));
        }
        HIP_TRY(hipStreamSynchronize(s));
        if (np) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, e[0], e[1]));
            st[23] += ms;
        }
        kept.resize(nk);
        for (int64_t i = 0; i < nk; ++i) kept[i] = {h_kidx[i], h_kbytes[i]};
        if ((rc = D.run(d_buf, d_offs, kept, &P->unmapped, s))) return rc;
        for (int64_t i = 0; i < nk; ++i) st[25] += (double)h_kbytes[i];
        // pairs by window (input order), then file order; the spanning ones get their text
        order.resize(np);
        for (int64_t p = 0; p < np; ++p) order[p] = p;
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
            const int32_t wa = W.order[h_pwin[a]], wb = W.order[h_pwin[b]];
            return wa != wb ? wa < wb : h_prec[a] < h_prec[b];
        });
        t_rec.clear(); t_rs.clear(); t_end.clear(); t_toff.assign(1, 0);
        const size_t p0 = P->pairs.size() / SPAN_FIELDS;
        P->pairs.resize(P->pairs.size() + np * SPAN_FIELDS);
        for (int64_t j = 0; j < np; ++j) {
            const size_t p = order[j];
            const int64_t *o = h_out.data() + bam::SPAN_OUT * p;
            const int32_t w = W.order[h_pwin[p]];
            bam::Span sp = {(int32_t)o[0], o[1], o[2], o[3], o[4], o[5]};
            if (sp.status == bam::SPAN_CG_TAG) {
                int64_t ro = 0;
                uint8_t head[36 + 256];
                HIP_TRY(hipMemcpy(&ro, d_offs + h_prec[p], 8, hipMemcpyDeviceToHost));
                HIP_TRY(hipMemcpy(head, d_buf + ro, 36 + o[6], hipMemcpyDeviceToHost));
                return cg_error("", std::string((const char *)head + 36, o[6]), (long long)(at + ro));
            }
            put_pair(P->pairs.data() + SPAN_FIELDS * (p0 + j), w, win_locus[w], records_before + h_prec[p], sp, o[6]);
            if (sp.status == bam::SPAN_OK) {
                t_rec.push_back(h_prec[p]);
                t_rs.push_back(sp.rs);
                t_end.push_back(sp.end);
                t_toff.push_back(t_toff.back() + o[6] + sp.end - sp.rs);
                st[17] += 1;
            } else {
                st[17 + sp.status] += 1;
            }
            P->text_off.push_back(P->text.size() + t_toff.back());
        }
        st[16] += (double)np;
        const int64_t nt = (int64_t)t_rec.size(), bytes = t_toff.back();
        if (nt) {
            if ((rc = d_trec.ensure(nt)) || (rc = d_trs.ensure(nt)) || (rc = d_tend.ensure(nt)) || (rc = d_ttoff.ensure(nt + 1)) ||
                (rc = d_text.ensure((size_t)std::max<int64_t>(1, bytes))))
                return rc;
            HIP_TRY(hipMemcpyAsync(d_trec.p, t_rec.data(), nt * 8, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(d_trs.p, t_rs.data(), nt * 8, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(d_tend.p, t_end.data(), nt * 8, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(d_ttoff.p, t_toff.data(), (nt + 1) * 8, hipMemcpyHostToDevice, s));
            HIP_TRY(hipEventRecord(e[2], s));
            hipLaunchKernelGGL(bam::trim_decode_kernel, dim3((unsigned)((nt + 3) / 4)), dim3(256), 0, s, d_buf, d_offs, d_trec.p,
                               d_trs.p, d_tend.p, d_ttoff.p, nt, d_text.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(e[3], s));
            const size_t t0 = P->text.size();
            P->text.resize(t0 + bytes);
            if (bytes) HIP_TRY(hipMemcpyAsync(P->text.data() + t0, d_text.p, bytes, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, e[2], e[3]));
            st[27] += ms;
            st[24] += (double)bytes;
        }
        return ADVNTR_OK;
    };
    (void)current_device();
    for (int i = 0; i < 4; ++i)
        if (hipEventCreate(&e[i]) != hipSuccess) return fail(ADVNTR_ERR_DEVICE, "%s: hipEventCreate failed", who), nullptr;
    if (hipMemcpy(d_win_ptr.p, wp.data(), wp.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        (n_win && (hipMemcpy(d_ws.p, W.start.data(), n_win * 8, hipMemcpyHostToDevice) != hipSuccess ||
                   hipMemcpy(d_we.p, W.end.data(), n_win * 8, hipMemcpyHostToDevice) != hipSuccess ||
                   hipMemcpy(d_wmax.p, W.maxend.data(), n_win * 8, hipMemcpyHostToDevice) != hipSuccess)))
        return fail(ADVNTR_ERR_DEVICE, "%s: window upload failed", who), nullptr;
    std::vector<int64_t> no_offsets;
    if (bam_stream(who, path, n_ref, chunk_bytes, false, no_offsets, st, spans)) return nullptr;
    st[4] = P->unmapped.stats[4];
    // chunks come in file order, each sorted by window then record: a stable sort by window orders the whole pass
    const int64_t np = (int64_t)P->pairs.size() / SPAN_FIELDS;
    order.resize(np);
    for (int64_t p = 0; p < np; ++p) order[p] = p;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return P->pairs[SPAN_FIELDS * a] < P->pairs[SPAN_FIELDS * b]; });
    std::vector<int64_t> pairs(P->pairs.size()), toff(np + 1, 0);
    std::vector<uint8_t> text(P->text.size());
    for (int64_t j = 0; j < np; ++j) {
        const size_t p = order[j];
        std::copy(P->pairs.begin() + SPAN_FIELDS * p, P->pairs.begin() + SPAN_FIELDS * (p + 1), pairs.begin() + SPAN_FIELDS * j);
        const int64_t a = P->text_off[p], z = P->text_off[p + 1];
        std::copy(P->text.begin() + a, P->text.begin() + z, text.begin() + toff[j]);
        toff[j + 1] = toff[j] + (z - a);
    }
    P->pairs.swap(pairs);
    P->text.swap(text);
    P->text_off.swap(toff);
    (void)flags;
    return P.release();
}

extern "C" int advntr_bam_spans_info(const advntr_bam_spans *P, int64_t *n_pairs, int64_t *text_bytes, int64_t *n_unmapped,
                                     int64_t *unmapped_text_bytes, double *stats)
{
    if (!P) return fail(ADVNTR_ERR_ARG, "advntr_bam_spans_info: null handle");
    if (n_pairs) *n_pairs = (int64_t)P->pairs.size() / SPAN_FIELDS;
    if (text_bytes) *text_bytes = (int64_t)P->text.size();
    if (n_unmapped) *n_unmapped = (int64_t)P->unmapped.text_off.size() - 1;
    if (unmapped_text_bytes) *unmapped_text_bytes = (int64_t)P->unmapped.text.size();
    if (stats) std::copy(P->stats, P->stats + ADVNTR_BAM_SPAN_STATS, stats);
    return ADVNTR_OK;
}

extern "C" int advntr_bam_spans_fetch(const advntr_bam_spans *P, int64_t *pairs, uint8_t *text, int64_t *text_off, int32_t *fields,
                                      uint8_t *unmapped_text, int64_t *unmapped_text_off)
{
    if (!P) return fail(ADVNTR_ERR_ARG, "advntr_bam_spans_fetch: null handle");
    if (pairs) std::copy(P->pairs.begin(), P->pairs.end(), pairs);
    if (text) std::copy(P->text.begin(), P->text.end(), text);
    if (text_off) std::copy(P->text_off.begin(), P->text_off.end(), text_off);
    return advntr_bam_kept_fetch(&P->unmapped, fields, unmapped_text, unmapped_text_off);
}

extern "C" void advntr_bam_spans_destroy(advntr_bam_spans *P) { delete P; }
