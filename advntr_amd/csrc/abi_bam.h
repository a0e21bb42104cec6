// abi_bam.h -- C-ABI entry points of the BAM input (bgzf_inflate.h, bam_records.h).  Included by engine.hip.
#pragma once
#include <cstdio>
#include "bgzf_inflate.h"
#include "bam_records.h"

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

}  // namespace

struct advntr_bam_kept {
    std::vector<int32_t> fields;
    std::vector<uint8_t> text;
    std::vector<int64_t> text_off{0};
    std::vector<int64_t> offsets;
    double stats[ADVNTR_BAM_STATS] = {0};
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

extern "C" advntr_bam_kept *advntr_bam_select(const char *path, int32_t n_ref, const int32_t *win_ptr, const int64_t *win_start,
                                              const int64_t *win_end, int64_t chunk_bytes, uint32_t flags)
{
    const auto t_all = std::chrono::steady_clock::now();
    if (!path || n_ref < 0 || (n_ref && !win_ptr)) return fail(ADVNTR_ERR_ARG, "advntr_bam_select: bad argument"), nullptr;
    const int32_t n_win = n_ref ? win_ptr[n_ref] : 0;
    if (n_win < 0 || (n_win && (!win_start || !win_end))) return fail(ADVNTR_ERR_ARG, "advntr_bam_select: bad windows"), nullptr;
    if (advntr_device_count() <= 0) return fail(ADVNTR_ERR_DEVICE, "advntr_bam_select: no HIP device visible (no CPU fallback)"), nullptr;
    // windows per reference sorted by start, with the running maximum of their ends
    std::vector<int64_t> ws(n_win), wmax(n_win);
    for (int32_t r = 0; r < n_ref; ++r) {
        if (win_ptr[r + 1] < win_ptr[r]) return fail(ADVNTR_ERR_ARG, "advntr_bam_select: win_ptr not monotone"), nullptr;
        std::vector<std::pair<int64_t, int64_t>> w;
        for (int32_t k = win_ptr[r]; k < win_ptr[r + 1]; ++k) w.emplace_back(win_start[k], win_end[k]);
        std::sort(w.begin(), w.end());
        int64_t m = INT64_MIN;
        for (size_t k = 0; k < w.size(); ++k) {
            ws[win_ptr[r] + k] = w[k].first;
            wmax[win_ptr[r] + k] = m = std::max(m, w[k].second);
        }
    }
    BamHeader H;
    if (read_bam_header(path, H)) return nullptr;
    if ((int32_t)H.names.size() != n_ref)
        return fail(ADVNTR_ERR_ARG, "advntr_bam_select: %d window lists for %d references", n_ref, (int)H.names.size()), nullptr;

    std::unique_ptr<advntr_bam_kept> K(new advntr_bam_kept());
    double *st = K->stats;
    BamScan S;
    S.path = path;
    S.chunk = chunk_bytes > 0 ? chunk_bytes : (int64_t)256 << 20;
    S.f = fopen(path, "rb");
    if (!S.f) return fail(ADVNTR_ERR_ARG, "cannot open %s", path), nullptr;
    (void)current_device();
#define BAM_TRY(expr)                                                                                                     \
    do {                                                                                                                  \
        hipError_t e_ = (expr);                                                                                           \
        if (e_ != hipSuccess) return fail(ADVNTR_ERR_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_)), nullptr;    \
    } while (0)
#define BAM_RC(expr)                                                                                                      \
    do {                                                                                                                  \
        if ((expr) != ADVNTR_OK) return nullptr;                                                                          \
    } while (0)
    BAM_TRY(hipStreamCreateWithFlags(&S.s_copy, hipStreamNonBlocking));
    BAM_TRY(hipStreamCreateWithFlags(&S.s_run, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
        BAM_TRY(hipHostMalloc((void **)&S.pinned[i], (size_t)(S.chunk + 65536), hipHostMallocDefault));
        BAM_TRY(hipEventCreate(&S.uploaded[i]));
        BAM_TRY(hipEventCreate(&S.up_t0[i]));
    }
    BAM_TRY(hipEventCreate(&S.k_t0));
    BAM_TRY(hipEventCreate(&S.k_t1));
    DevBuf<int32_t> d_win_ptr, d_count;
    DevBuf<int64_t> d_ws, d_wmax, d_start, d_stop, d_end, d_base, d_offs, d_kidx, d_kbytes, d_toff;
    DevBuf<unsigned long long> d_counters;
    DevBuf<int32_t> d_fields;
    DevBuf<uint8_t> d_text;
    BAM_RC(d_win_ptr.ensure(n_ref + 1));
    BAM_RC(d_ws.ensure(n_win));
    BAM_RC(d_wmax.ensure(n_win));
    BAM_RC(d_counters.ensure(2));
    std::vector<int32_t> wp(win_ptr, win_ptr + n_ref + 1);
    if (!n_ref) wp.assign(1, 0);
    BAM_TRY(hipMemcpy(d_win_ptr.p, wp.data(), wp.size() * 4, hipMemcpyHostToDevice));
    if (n_win) {
        BAM_TRY(hipMemcpy(d_ws.p, ws.data(), n_win * 8, hipMemcpyHostToDevice));
        BAM_TRY(hipMemcpy(d_wmax.p, wmax.data(), n_win * 8, hipMemcpyHostToDevice));
    }
    InflateLaunch L;
    int64_t uncompressed_before = 0;    // uncompressed bytes of the blocks before the current chunk
    int64_t records_before = 0, carry = 0;
    std::vector<int64_t> h_start, h_stop, h_end, h_base, h_kidx, h_kbytes, h_toff, h_offs;
    std::vector<int32_t> h_count, h_fields;
    std::vector<std::pair<int64_t, int64_t>> kept;
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
        BAM_TRY(hipStreamWaitEvent(S.s_run, S.uploaded[slot], 0));
        BAM_TRY(hipEventRecord(S.k_t0, S.s_run));
        BAM_RC(L.launch(B, S.blocks[slot].front().off, S.d_comp[slot].p, carry, d_buf, S.s_run));
        BAM_TRY(hipEventRecord(S.k_t1, S.s_run));
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
        BAM_TRY(hipMemcpyAsync(d_start.p, h_start.data(), nb * 8, hipMemcpyHostToDevice, S.s_run));
        BAM_TRY(hipMemcpyAsync(d_stop.p, h_stop.data(), nb * 8, hipMemcpyHostToDevice, S.s_run));
        hipLaunchKernelGGL(bam::walk_blocks_kernel, dim3((nb + 255) / 256), dim3(256), 0, S.s_run, d_buf, buflen, d_start.p, d_stop.p,
                           nb, d_end.p, d_count.p, (const int64_t *)nullptr, (int64_t *)nullptr);
        BAM_TRY(hipGetLastError());
        BAM_TRY(hipMemcpyAsync(h_end.data(), d_end.p, nb * 8, hipMemcpyDeviceToHost, S.s_run));
        BAM_TRY(hipMemcpyAsync(h_count.data(), d_count.p, nb * 4, hipMemcpyDeviceToHost, S.s_run));
        // the next chunk is read, framed and uploaded while this one's kernels run
        BAM_RC(S.prepare(slot ^ 1, slot, st));
        BAM_RC(L.check(B, S.s_run));         // synchronises s_run
        {
            float ms = 0;
            BAM_TRY(hipEventElapsedTime(&ms, S.k_t0, S.k_t1));
            st[9] += ms;
            BAM_TRY(hipEventSynchronize(S.uploaded[slot]));
            BAM_TRY(hipEventElapsedTime(&ms, S.up_t0[slot], S.uploaded[slot]));
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
                if (fetch_window(s, std::min(buflen, std::max(s, h_stop[b]) + 4))) return nullptr;
                int64_t p = s, c = 0;
                while (p < h_stop[b] && p + 4 <= buflen) {
                    const int32_t bs = bam::rd_i32(window.data() + (p - lo));
                    if (bs < bam::MIN_RECORD)
                        return fail(ADVNTR_ERR_DATA, "%s: BAM record with block_size %d at uncompressed offset %lld", path, bs,
                                    (long long)(uncompressed_before - carry + p)), nullptr;
                    if (p + 4 + (int64_t)bs > buflen) break;
                    ++c;
                    p += 4 + (int64_t)bs;
                    if (p < h_stop[b] && fetch_window(p, std::min(buflen, h_stop[b] + 4))) return nullptr;
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
            BAM_TRY(hipMemcpyAsync(d_start.p, h_start.data(), nb * 8, hipMemcpyHostToDevice, S.s_run));
            BAM_TRY(hipMemcpyAsync(d_count.p, h_count.data(), nb * 4, hipMemcpyHostToDevice, S.s_run));
            BAM_TRY(hipMemcpyAsync(d_base.p, h_base.data(), nb * 8, hipMemcpyHostToDevice, S.s_run));
            hipLaunchKernelGGL(bam::walk_blocks_kernel, dim3((nb + 255) / 256), dim3(256), 0, S.s_run, d_buf, buflen, d_start.p,
                               d_stop.p, nb, d_end.p, d_count.p, d_base.p, d_offs.p);
            BAM_TRY(hipGetLastError());
            if (flags & ADVNTR_BAM_RECORD_OFFSETS) {
                h_offs.resize(n_rec);
                BAM_TRY(hipMemcpyAsync(h_offs.data(), d_offs.p, n_rec * 8, hipMemcpyDeviceToHost, S.s_run));
                BAM_TRY(hipStreamSynchronize(S.s_run));
                for (int64_t i = 0; i < n_rec; ++i) K->offsets.push_back(uncompressed_before - carry + h_offs[i]);
            }
        }
        BAM_TRY(hipStreamSynchronize(S.s_run));
        st[10] += ms_since(t_walk);
        const auto t_sel = std::chrono::steady_clock::now();
        if (n_rec) {
            BAM_RC(d_kidx.ensure(n_rec));
            BAM_RC(d_kbytes.ensure(n_rec));
            const unsigned long long init[2] = {0, ~0ull};
            BAM_TRY(hipMemcpyAsync(d_counters.p, init, sizeof init, hipMemcpyHostToDevice, S.s_run));
            hipLaunchKernelGGL(bam::select_kernel, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, S.s_run, d_buf, d_offs.p, n_rec,
                               std::max<int64_t>(0, 5 - records_before), n_ref, d_win_ptr.p, d_ws.p, d_wmax.p, d_counters.p,
                               d_kidx.p, d_kbytes.p, n_rec, d_counters.p + 1);
            BAM_TRY(hipGetLastError());
            unsigned long long cnt[2];
            BAM_TRY(hipMemcpyAsync(cnt, d_counters.p, sizeof cnt, hipMemcpyDeviceToHost, S.s_run));
            BAM_TRY(hipStreamSynchronize(S.s_run));
            if (cnt[1] != ~0ull) {
                h_offs.resize(n_rec);
                BAM_TRY(hipMemcpy(h_offs.data(), d_offs.p, n_rec * 8, hipMemcpyDeviceToHost));
                return fail(ADVNTR_ERR_DATA, "%s: malformed BAM record at uncompressed offset %lld", path,
                            (long long)(uncompressed_before - carry + h_offs[cnt[1]])), nullptr;
            }
            const int64_t nk = (int64_t)cnt[0];
            if (nk) {
                h_kidx.resize(nk); h_kbytes.resize(nk);
                BAM_TRY(hipMemcpy(h_kidx.data(), d_kidx.p, nk * 8, hipMemcpyDeviceToHost));
                BAM_TRY(hipMemcpy(h_kbytes.data(), d_kbytes.p, nk * 8, hipMemcpyDeviceToHost));
                kept.resize(nk);
                for (int64_t i = 0; i < nk; ++i) kept[i] = {h_kidx[i], h_kbytes[i]};
                std::sort(kept.begin(), kept.end());
                h_toff.resize(nk + 1);
                h_toff[0] = 0;
                for (int64_t i = 0; i < nk; ++i) {
                    h_kidx[i] = kept[i].first;
                    h_toff[i + 1] = h_toff[i] + kept[i].second;
                }
                BAM_RC(d_toff.ensure(nk + 1));
                BAM_RC(d_fields.ensure(nk * bam::FIELDS));
                BAM_RC(d_text.ensure((size_t)std::max<int64_t>(1, h_toff[nk])));
                BAM_TRY(hipMemcpyAsync(d_kidx.p, h_kidx.data(), nk * 8, hipMemcpyHostToDevice, S.s_run));
                BAM_TRY(hipMemcpyAsync(d_toff.p, h_toff.data(), (nk + 1) * 8, hipMemcpyHostToDevice, S.s_run));
                hipLaunchKernelGGL(bam::decode_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, S.s_run, d_buf, d_offs.p,
                                   d_kidx.p, d_toff.p, nk, d_fields.p, d_text.p);
                BAM_TRY(hipGetLastError());
                const size_t f0 = K->fields.size(), t0 = K->text.size();
                K->fields.resize(f0 + nk * bam::FIELDS);
                K->text.resize(t0 + h_toff[nk]);
                BAM_TRY(hipMemcpyAsync(K->fields.data() + f0, d_fields.p, nk * bam::FIELDS * 4, hipMemcpyDeviceToHost, S.s_run));
                if (h_toff[nk]) BAM_TRY(hipMemcpyAsync(K->text.data() + t0, d_text.p, h_toff[nk], hipMemcpyDeviceToHost, S.s_run));
                BAM_TRY(hipStreamSynchronize(S.s_run));
                for (int64_t i = 0; i < nk; ++i) K->text_off.push_back((int64_t)t0 + h_toff[i + 1]);
                st[4] += (double)nk;
            }
        }
        st[13] += ms_since(t_sel);
        // the bytes of the record that did not fit go to the front of the next chunk's output
        const std::vector<BgzfBlock> &N = S.blocks[slot ^ 1];
        if (N.empty() && carry_next > 0)
            return fail(ADVNTR_ERR_DATA, "%s: the file ends inside a BAM record (uncompressed offset %lld)", path,
                        (long long)(uncompressed_before - carry + s)), nullptr;
        int64_t next_isum = 0;
        for (const BgzfBlock &b : N) next_isum += b.isize;
        BAM_RC(S.d_out[slot ^ 1].ensure((size_t)std::max<int64_t>(1, carry_next + next_isum)));
        if (carry_next)
            BAM_TRY(hipMemcpyAsync(S.d_out[slot ^ 1].p, d_buf + s, (size_t)carry_next, hipMemcpyDeviceToDevice, S.s_run));
        st[0] += nb;
        st[1] += (double)(B.back().off + B.back().bytes - B.front().off);
        st[2] += (double)isum;
        st[3] += (double)n_rec;
        st[5] += 1;
        records_before += n_rec;
        uncompressed_before += isum;
        carry = carry_next;
    }
    BAM_TRY(hipStreamSynchronize(S.s_run));
    if (H.bytes > uncompressed_before) return fail(ADVNTR_ERR_DATA, "%s: the file ends inside the BAM header", path), nullptr;
    st[14] = ms_since(t_all);
#undef BAM_TRY
#undef BAM_RC
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
