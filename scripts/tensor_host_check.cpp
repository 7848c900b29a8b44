// Runs the tensor arithmetic of megapath_nano_amd/csrc/tensor_core.h on the CPU, serially -- the record facts tens_records_kernel
// computes, the join test of tens_join_kernel, the centre flag and the fill a wave computes -- so that every test case, malformed
// records included, has been through the bounds decisions under the host's tools before it meets a GPU:
//
//   g++ -O1 -g -fsanitize=address,undefined -o tensor_host_check scripts/tensor_host_check.cpp
//   tensor_host_check cases.bin results.bin
//
// cases.bin:   u32 n, then per case u64 text length, i64 ref_start, u64 ref_len, i32 left_edge, u32 rows, u32 centres, the text,
//              the reference bytes, then per row i64 off, then per centre i32 c0, u32 begin, u32 end (the rows that are looked at).
// results.bin: per case, per row the 16 bytes of mpn_tensor_rec (status 255: the row's fixed bytes do not lie inside the text),
//              i64 span, i32 pos, i32 reverse; then per centre, per row of its range u8 joins, i8 flag (0 if it does not join),
//              i16 rc of the fill (-1: does not join), and then the 1056 int32 of the tensor of all the rows that join.
// The text and the reference are heap blocks of their exact size: a read outside them is reported.  Built with -O2 it is also
// the serial baseline of scripts/bench_create_tensor.py (it prints the seconds spent on centres to standard error).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../megapath_nano_amd/csrc/tensor_core.h"

using namespace mpn_tens;

static bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

struct Row { int64_t off, span; int32_t pos, reverse; bool inside; };

int main(int argc, char **argv) {
    static_assert(sizeof(mpn_tensor_rec) == 16, "the layout of the result file");
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]); return 2; }
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) { perror("open"); return 2; }
    uint32_t n = 0;
    if (!read_exact(fi, &n, 4)) { fprintf(stderr, "short case file\n"); return 2; }
    double seconds = 0;
    for (uint32_t c = 0; c < n; ++c) {
        uint64_t len = 0, ref_len = 0;
        int64_t ref_start = 0;
        int32_t left_edge = 1;
        uint32_t n_rows = 0, n_centres = 0;
        if (!read_exact(fi, &len, 8) || !read_exact(fi, &ref_start, 8) || !read_exact(fi, &ref_len, 8) || !read_exact(fi, &left_edge, 4) ||
            !read_exact(fi, &n_rows, 4) || !read_exact(fi, &n_centres, 4)) {
            fprintf(stderr, "bad case file\n");
            return 2;
        }
        std::unique_ptr<uint8_t[]> text(new uint8_t[len]), ref(new uint8_t[ref_len]);
        if (!read_exact(fi, text.get(), len) || !read_exact(fi, ref.get(), ref_len)) { fprintf(stderr, "short case file\n"); return 2; }
        std::vector<Row> rows(n_rows);
        for (Row &r : rows) {
            if (!read_exact(fi, &r.off, 8)) { fprintf(stderr, "short case file\n"); return 2; }
            mpn_tensor_rec rec;
            memset(&rec, 0, sizeof rec);
            r.span = 0; r.pos = 0; r.reverse = 0;
            r.inside = !(r.off < 0 || r.off > (int64_t)len - BAMW_FIXED);
            if (!r.inside) {
                rec.status = 255;
            } else {
                tens_record(text.get(), (int64_t)len, r.off, &rec);
                mpn_pileup_rec p;
                pile_record(text.get(), (int64_t)len, r.off, &p);
                r.span = p.status == MPN_PILEUP_OK || p.status == MPN_PILEUP_NO_BASE ? p.span : 0;
                r.pos = p.pos;
                r.reverse = (bamw_u16(text.get(), r.off + 18) & 16) ? 1 : 0;
            }
            fwrite(&rec, sizeof rec, 1, fo);
            fwrite(&r.span, 8, 1, fo);
            fwrite(&r.pos, 4, 1, fo);
            fwrite(&r.reverse, 4, 1, fo);
        }
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t k = 0; k < n_centres; ++k) {
            int32_t c0 = 0;
            uint32_t begin = 0, end = 0;
            if (!read_exact(fi, &c0, 4) || !read_exact(fi, &begin, 4) || !read_exact(fi, &end, 4) || begin > end || end > n_rows) {
                fprintf(stderr, "bad case file\n");
                return 2;
            }
            int32_t tile[CELLS];
            memset(tile, 0, sizeof tile);
            for (uint32_t i = begin; i < end; ++i) {
                const Row &r = rows[i];
                const uint8_t joins = r.inside && tens_joins(r.pos, r.span, c0, left_edge) ? 1 : 0;
                int8_t flag = 0;
                int16_t rc = -1;
                if (joins) {
                    flag = (int8_t)tens_flag_serial(text.get(), (int64_t)len, r.off, r.pos, c0, left_edge);
                    rc = (int16_t)tens_fill_serial(text.get(), (int64_t)len, r.off, r.pos, r.reverse, c0, left_edge, ref.get(), ref_start, (int64_t)ref_len, tile);
                }
                fwrite(&joins, 1, 1, fo);
                fwrite(&flag, 1, 1, fo);
                fwrite(&rc, 2, 1, fo);
            }
            fwrite(tile, 4, CELLS, fo);
        }
        seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    fprintf(stderr, "centres: %.6f s\n", seconds);
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 1;
}
