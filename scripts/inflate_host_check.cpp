// Runs gzip streams through the serial decoder of megapath_nano_amd/csrc/inflate_core.h on the CPU -- the code one lane of
// gzip_inflate_kernel runs, with the flush done by one thread -- so that every test case, malformed ones included, has been
// through the bounds decisions under the host's tools before it meets a GPU:
//
//   g++ -O1 -g -fsanitize=address,undefined -o inflate_host_check scripts/inflate_host_check.cpp
//   inflate_host_check cases.bin results.bin
//
// cases.bin:   u32 n, then per case u64 input length, u64 slot capacity, the input bytes.
// results.bin: per case i32 status, i32 members, u64 inflated length, u64 bytes stored (min(length, capacity)), those bytes.
// Input, ring, code tables and slot are heap blocks of their exact sizes: a read or write outside them is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../megapath_nano_amd/csrc/inflate_core.h"

using namespace mpn_inf;

static bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]); return 2; }
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) { perror("open"); return 2; }
    uint32_t n = 0;
    if (!read_exact(fi, &n, 4)) { fprintf(stderr, "short case file\n"); return 2; }
    for (uint32_t c = 0; c < n; ++c) {
        uint64_t in_len = 0, cap = 0;
        if (!read_exact(fi, &in_len, 8) || !read_exact(fi, &cap, 8)) { fprintf(stderr, "short case file\n"); return 2; }
        std::unique_ptr<uint8_t[]> in(new uint8_t[in_len]), slot(new uint8_t[cap]), ring(new uint8_t[INF_WIN]), lens(new uint8_t[INF_MAX_LENS]);
        std::unique_ptr<InfCode> ll(new InfCode), dc(new InfCode);
        if (!read_exact(fi, in.get(), in_len)) { fprintf(stderr, "short case file\n"); return 2; }
        memset(ring.get(), 0, INF_WIN);
        InfState st;
        inf_init(&st, 0, (int64_t)in_len);
        bool finished = false;
        const int64_t max_calls = inf_max_calls((int64_t)in_len);
        for (int64_t it = 0; it < max_calls && !finished; ++it) {
            finished = inf_run(&st, in.get(), ring.get(), ll.get(), dc.get(), lens.get()) != 0;
            inf_flush_serial(&st, ring.get(), slot.get(), (int64_t)cap);
        }
        const int32_t status = finished ? inf_final_status(&st, (int64_t)cap) : MPN_INFLATE_TRUNCATED, members = st.members;
        const uint64_t out_len = (uint64_t)st.out_pos, stored = out_len < cap ? out_len : cap;
        fwrite(&status, 4, 1, fo);
        fwrite(&members, 4, 1, fo);
        fwrite(&out_len, 8, 1, fo);
        fwrite(&stored, 8, 1, fo);
        if (stored) fwrite(slot.get(), 1, stored, fo);
    }
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 1;
}
