// Builds name sets with ns_build and probes them with ns_hash / ns_probe of megapath_nano_amd/csrc/name_set_core.h on the CPU -- the
// functions a lane of name_lookup_kernel calls -- so that every case of names has been through the table's bounds decisions under
// the host's tools before it meets a GPU:
//
//   g++ -O1 -g -fsanitize=address,undefined -o name_set_host_check scripts/name_set_host_check.cpp
//   name_set_host_check cases.bin results.bin
//
// cases.bin:   u32 cases, then per case i64 slots, u64 n names, per name u64 length + bytes, u64 q queries, per query u64 length + bytes.
// results.bin: per case i32 rc of ns_build; for rc = 0: i64 slots of the table, i64 distinct names, n x i32 first_of, and per query
//              i32 found, i32 slots read.
// The name pool and every query are heap blocks of their exact sizes: a read outside them is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../megapath_nano_amd/csrc/name_set_core.h"

using namespace mpn;

static bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static void short_file() { fprintf(stderr, "short case file\n"); exit(2); }

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]); return 2; }
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) { perror("open"); return 2; }
    uint32_t cases = 0;
    if (!read_exact(fi, &cases, 4)) short_file();
    for (uint32_t c = 0; c < cases; ++c) {
        int64_t slots = 0;
        uint64_t n = 0, q = 0;
        if (!read_exact(fi, &slots, 8) || !read_exact(fi, &n, 8)) short_file();
        std::vector<int64_t> off(n + 1, 0);
        std::vector<char> grow;
        for (uint64_t i = 0; i < n; ++i) {
            uint64_t len = 0;
            if (!read_exact(fi, &len, 8)) short_file();
            grow.resize(grow.size() + len);
            if (!read_exact(fi, grow.data() + off[i], len)) short_file();
            off[i + 1] = off[i] + (int64_t)len;
        }
        std::unique_ptr<char[]> pool(new char[grow.size()]);     // (exact size: a vector may own more)
        if (!grow.empty()) memcpy(pool.get(), grow.data(), grow.size());
        NsBuilt built;
        std::vector<int32_t> first_of(n, -7);
        const char *what = "";
        const int32_t rc = ns_build((int64_t)n, pool.get(), off.data(), slots, built, first_of.data(), &what);
        fwrite(&rc, 4, 1, fo);
        if (rc == 0) {
            const int64_t got_slots = (int64_t)built.table.size();
            fwrite(&got_slots, 8, 1, fo);
            fwrite(&built.distinct, 8, 1, fo);
            if (n) fwrite(first_of.data(), 4, n, fo);
        }
        if (!read_exact(fi, &q, 8)) short_file();
        for (uint64_t k = 0; k < q; ++k) {
            uint64_t len = 0;
            if (!read_exact(fi, &len, 8)) short_file();
            std::unique_ptr<uint8_t[]> id(new uint8_t[len]);
            if (!read_exact(fi, id.get(), len)) short_file();
            if (rc) continue;
            const NsHostBytes words{id.get(), (int32_t)len};
            uint32_t at = 0;
            int64_t probes = 0;
            const int32_t found = ns_probe(built.table.data(), (uint32_t)(built.table.size() - 1), ns_hash((int32_t)len, words), (int32_t)len, words,
                                           NsHostPool{built.pool.data()}, &at, &probes);
            const int32_t seen = (int32_t)probes;
            fwrite(&found, 4, 1, fo);
            fwrite(&seen, 4, 1, fo);
        }
    }
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 1;
}
