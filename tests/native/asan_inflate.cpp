// The __host__ __device__ inflate core (advntr_amd/csrc/bgzf_inflate.h) on the CPU, built by tests/test_bam_cpu.py with plain
// g++ under -fsanitize=address,undefined.  Input file: cases of (u32 in_len, u32 out_cap, in_len bytes).  Output file: per case
// (i32 status, u32 out_len, out_len bytes).  Each case gets buffers of exactly its size, so any read past the compressed span
// or write past the capacity is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../advntr_amd/csrc/bgzf_inflate.h"

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    bgzf::Tables *T = new bgzf::Tables;
    bgzf::HostWave w;
    bgzf::fill_crc_table(*T, w);
    uint32_t hdr[2];
    int cases = 0;
    while (fread(hdr, 4, 2, in) == 2) {
        std::vector<uint8_t> src(hdr[0]);
        if (hdr[0] && fread(src.data(), 1, hdr[0], in) != hdr[0]) return 3;
        uint8_t *a = (uint8_t *)malloc(hdr[0] ? hdr[0] : 1), *o = (uint8_t *)malloc(hdr[1] ? hdr[1] : 1);
        std::copy(src.begin(), src.end(), a);
        uint32_t got = 0;
        int32_t rc = bgzf::inflate_raw(a, hdr[0], o, hdr[1], &got, *T, w);
        // the CRC path of the core as well (crc32_wave with one lane is the plain table CRC)
        uint32_t scratch[2];
        const uint32_t crc = bgzf::crc32_wave(*T, o, got, w, scratch);
        if (crc != bgzf::crc32_combine(bgzf::crc32_bytes(T->crc, o, got / 2), bgzf::crc32_bytes(T->crc, o + got / 2, got - got / 2),
                                       got - got / 2))
            return 4;
        fwrite(&rc, 4, 1, out);
        fwrite(&got, 4, 1, out);
        fwrite(o, 1, got, out);
        free(a);
        free(o);
        ++cases;
    }
    delete T;
    fclose(out);
    fclose(in);
    printf("ok %d\n", cases);
    return 0;
}
