// Runs the device BAM writer's rules (megapath_nano_amd/csrc/bam_out_core.h) serially on the CPU -- scan and encode of SAM lines, the
// BGZF block cut and the BAI builder, the very functions the kernels and mpn_bam_out_finish call -- so that every case has been
// through their bounds decisions under the host's tools before it meets a GPU:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -o bam_out_host_check scripts/bam_out_host_check.cpp
//   bam_out_host_check encode cases.bin results.bin
//   bam_out_host_check index cases.bin results.bin
//
// encode cases:   u32 references, per reference u32 length + bytes; i32 exclude_flags; u32 lines, per line u32 length + bytes.
// encode results: per line i32 status, tid, pos0, end0, flag, size, then the record's bytes.
// index cases:    u32 cases, per case i32 references, i64 header bytes, i64 records, per record i32 tid, pos0, end0, size, mapped.
// index results:  per case i64 blocks, (blocks + 1) x i64 block starts in the payload stream, u64 virtual offset of the first record
//                 and of the end, per record u64 virtual offset behind it (all provisional: block number << 16 | offset), then
//                 i64 bytes of the .bai + the bytes, built from the file addresses the blocks have in stored mode (payload + 31).
// Every line and every record is a heap block of its exact size: a read or write outside it is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../megapath_nano_amd/csrc/bam_out_core.h"
#include "../megapath_nano_amd/csrc/name_set_core.h"

using namespace mpn;
using namespace mpn::bo;

static FILE *fi, *fo;
template <typename T> static T get() {
    T v;
    if (fread(&v, sizeof(T), 1, fi) != 1) { fprintf(stderr, "short case file\n"); exit(2); }
    return v;
}
static void get_bytes(void *p, size_t n) {
    if (n && fread(p, 1, n, fi) != n) { fprintf(stderr, "short case file\n"); exit(2); }
}
template <typename T> static void put(T v) { fwrite(&v, sizeof(T), 1, fo); }

static int run_encode() {
    const uint32_t n_ref = get<uint32_t>();
    std::string pool;
    std::vector<int64_t> off(n_ref + 1, 0);
    for (uint32_t i = 0; i < n_ref; ++i) {
        const uint32_t len = get<uint32_t>();
        std::string s(len, '\0');
        get_bytes(&s[0], len);
        pool += s;
        off[i + 1] = (int64_t)pool.size();
    }
    NsBuilt set;
    const char *what = "";
    if (ns_build(n_ref, pool.data(), off.data(), 0, set, nullptr, &what)) { fprintf(stderr, "ns_build: %s\n", what); return 2; }
    const uint32_t mask = (uint32_t)(set.table.size() - 1);
    auto lookup = [&](const uint8_t *p, int32_t len) {
        const NsHostBytes id{p, len};
        return ns_find(set.table.data(), mask, ns_hash(len, id), len, id, NsHostPool{set.pool.data()});
    };
    const int32_t exclude = get<int32_t>();
    const uint32_t n = get<uint32_t>();
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t len = get<uint32_t>();
        std::unique_ptr<uint8_t[]> line(new uint8_t[len]);
        get_bytes(line.get(), len);
        int32_t tab[11] = {0};
        BoRec r;
        bo_scan_line(line.get(), (int32_t)len, exclude, lookup, tab, &r);
        put(r.status); put(r.tid); put(r.pos0); put(r.end0); put(r.flag); put(r.size);
        if (r.status == MPN_SAM_OK) {
            std::unique_ptr<uint8_t[]> rec(new uint8_t[r.size]);
            memset(rec.get(), 0xa5, (size_t)r.size);
            bo_encode_line(line.get(), (int32_t)len, tab, r, rec.get());
            fwrite(rec.get(), 1, (size_t)r.size, fo);
        }
    }
    return 0;
}

static int run_index() {
    const uint32_t cases = get<uint32_t>();
    for (uint32_t c = 0; c < cases; ++c) {
        const int32_t n_ref = get<int32_t>();
        const int64_t header = get<int64_t>(), n = get<int64_t>();
        std::vector<int32_t> tid((size_t)n), pos0((size_t)n), end0((size_t)n), size((size_t)n);
        std::vector<uint8_t> mapped((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            tid[(size_t)i] = get<int32_t>(); pos0[(size_t)i] = get<int32_t>(); end0[(size_t)i] = get<int32_t>(); size[(size_t)i] = get<int32_t>();
            mapped[(size_t)i] = (uint8_t)get<int32_t>();
        }
        BoCut cut;
        const uint64_t first = cut.header(header);
        std::vector<uint64_t> voff((size_t)n);
        for (int64_t i = 0; i < n; ++i) voff[(size_t)i] = cut.record(size[(size_t)i]);
        const uint64_t end = cut.close();
        const int64_t nb = cut.n_blocks();
        put(nb);
        fwrite(cut.block_start.data(), 8, (size_t)nb + 1, fo);
        put(first); put(end);
        if (n) fwrite(voff.data(), 8, (size_t)n, fo);
        std::vector<int64_t> addr((size_t)nb + 1, 0);
        for (int64_t b = 0; b < nb; ++b) addr[(size_t)b + 1] = addr[(size_t)b] + (cut.block_start[(size_t)b + 1] - cut.block_start[(size_t)b]) + 31;
        for (uint64_t &v : voff) v = bo_resolve(v, addr.data());
        const std::vector<uint8_t> bai = bai_build(n_ref, n, tid.data(), pos0.data(), end0.data(), voff.data(), mapped.data(), bo_resolve(first, addr.data()),
                                                   bo_resolve(end, addr.data()));
        put((int64_t)bai.size());
        fwrite(bai.data(), 1, bai.size(), fo);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 4 || (strcmp(argv[1], "encode") && strcmp(argv[1], "index"))) { fprintf(stderr, "usage: %s encode|index cases.bin results.bin\n", argv[0]); return 2; }
    fi = fopen(argv[2], "rb");
    fo = fopen(argv[3], "wb");
    if (!fi || !fo) { perror("open"); return 2; }
    const int rc = strcmp(argv[1], "encode") ? run_index() : run_encode();
    fclose(fi);
    if (fclose(fo) != 0) return 2;
    return rc;
}
