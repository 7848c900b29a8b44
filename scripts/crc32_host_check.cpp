// Takes the CRC-32 of byte strings with megapath_nano_amd/csrc/crc32_poly.h on the CPU, the way the kernels do it -- the byte
// table from crc_entry, a CRC from a zero register per slice, crc_slice for the bytes behind it, the xor over the slices, crc_join
// into the running register, flush after flush (bgzf_deflate_kernel stage E: 256 slices, one flush; inf_flush_wave: 64 slices, a
// flush per 16 KiB) -- so that the arithmetic is checked against zlib without a GPU and under the host's tools:
//
//   g++ -O1 -g -fsanitize=address,undefined -o crc32_host_check scripts/crc32_host_check.cpp
//   crc32_host_check cases.bin results.bin
//
// cases.bin:   u32 n, then per case u64 length, u64 split, u32 slices, the bytes.  The first flush is bytes [0, split), the second
//              [split, length); a flush without bytes is skipped, as the kernels skip it.
// results.bin: per case u32 CRC-32 (the final register, inverted).
// Every flush reads a heap block of its exact size: a read outside it is reported.
#include <cstdio>
#include <cstring>
#include <memory>

#include "../megapath_nano_amd/csrc/crc32_poly.h"

using namespace mpn_crc;

static bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static uint32_t flush(uint32_t reg, const uint8_t *src, uint32_t len, uint32_t slices, const uint32_t *tab) {
    if (len == 0) return reg;
    std::unique_ptr<uint8_t[]> p(new uint8_t[len]);
    memcpy(p.get(), src, len);
    const uint32_t per = (len + slices - 1) / slices;
    uint32_t parts = 0;
    for (uint32_t t = 0; t < slices; ++t) {
        const uint32_t a = t * per < len ? t * per : len, b = a + per < len ? a + per : len;
        uint32_t c = 0;
        for (uint32_t k = a; k < b; ++k) c = tab[(c ^ p[k]) & 0xff] ^ (c >> 8);
        parts ^= crc_slice(c, len - b);
    }
    return crc_join(reg, len, parts);
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]); return 2; }
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) { perror("open"); return 2; }
    uint32_t tab[256];
    for (uint32_t k = 0; k < 256; ++k) tab[k] = crc_entry(k);
    uint32_t n = 0;
    if (!read_exact(fi, &n, 4)) { fprintf(stderr, "short case file\n"); return 2; }
    for (uint32_t c = 0; c < n; ++c) {
        uint64_t len = 0, split = 0;
        uint32_t slices = 0;
        if (!read_exact(fi, &len, 8) || !read_exact(fi, &split, 8) || !read_exact(fi, &slices, 4) || split > len || slices == 0 ||
            len >= (1u << CRC_XPOW8_BITS)) {
            fprintf(stderr, "bad case file\n");
            return 2;
        }
        std::unique_ptr<uint8_t[]> data(new uint8_t[len]);
        if (!read_exact(fi, data.get(), len)) { fprintf(stderr, "short case file\n"); return 2; }
        uint32_t reg = 0xFFFFFFFFu;
        reg = flush(reg, data.get(), (uint32_t)split, slices, tab);
        reg = flush(reg, data.get() + split, (uint32_t)(len - split), slices, tab);
        const uint32_t crc = reg ^ 0xFFFFFFFFu;
        fwrite(&crc, 4, 1, fo);
    }
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 1;
}
