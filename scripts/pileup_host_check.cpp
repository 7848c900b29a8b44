// Runs the pile-up of megapath_nano_amd/csrc/pileup_core.h on the CPU, serially -- the record arithmetic pile_records_kernel runs,
// the counts a wave of pile_counts_kernel computes, the decision of the candidate kernels -- so that every test case, malformed
// records included, has been through the bounds decisions under the host's tools before it meets a GPU:
//
//   g++ -O1 -g -fsanitize=address,undefined -o pileup_host_check scripts/pileup_host_check.cpp
//   pileup_host_check cases.bin results.bin
//
// cases.bin:   u32 n, then per case u64 text length, i64 lo, i64 hi, f64 min_coverage, f64 threshold, u32 rows, the text, the
//              hi - lo reference bytes of the window, then per row i64 off, i32 take, i32 lead.
// results.bin: per case, per row the 40 bytes of mpn_pileup_rec (status 255: the row's fixed bytes do not lie inside the text) and
//              i32 rc of the counting (-1: not taken); then the (hi - lo) x 7 int32 counters; then u64 candidates and their
//              mpn_pileup_cand rows of 44 bytes.
// A taken row is counted at the pos its record says.  The text is a heap block of its exact size: a read outside it is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../megapath_nano_amd/csrc/pileup_core.h"

using namespace mpn_pile;

static bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
    static_assert(sizeof(mpn_pileup_rec) == 40 && sizeof(mpn_pileup_cand) == 44, "the layouts of the result file");
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]); return 2; }
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) { perror("open"); return 2; }
    uint32_t n = 0;
    if (!read_exact(fi, &n, 4)) { fprintf(stderr, "short case file\n"); return 2; }
    for (uint32_t c = 0; c < n; ++c) {
        uint64_t len = 0;
        int64_t lo = 0, hi = 0;
        double min_coverage = 0, threshold = 0;
        uint32_t n_rows = 0;
        if (!read_exact(fi, &len, 8) || !read_exact(fi, &lo, 8) || !read_exact(fi, &hi, 8) || !read_exact(fi, &min_coverage, 8) ||
            !read_exact(fi, &threshold, 8) || !read_exact(fi, &n_rows, 4) || lo < 0 || hi < lo || hi - lo > (1 << 24)) {
            fprintf(stderr, "bad case file\n");
            return 2;
        }
        std::unique_ptr<uint8_t[]> text(new uint8_t[len]), ref(new uint8_t[hi - lo]);
        if (!read_exact(fi, text.get(), len) || !read_exact(fi, ref.get(), (size_t)(hi - lo))) { fprintf(stderr, "short case file\n"); return 2; }
        std::vector<int32_t> counts((size_t)(hi - lo) * MPN_PILEUP_SLOTS, 0);
        for (uint32_t r = 0; r < n_rows; ++r) {
            int64_t off = 0;
            int32_t take = 0, lead = 0, rc = -1;
            if (!read_exact(fi, &off, 8) || !read_exact(fi, &take, 4) || !read_exact(fi, &lead, 4)) { fprintf(stderr, "short case file\n"); return 2; }
            mpn_pileup_rec rec;
            memset(&rec, 0, sizeof rec);
            if (off < 0 || off > (int64_t)len - BAMW_FIXED) {
                rec.status = 255;
            } else {
                pile_record(text.get(), (int64_t)len, off, &rec);
                if (take) rc = pile_count_serial(text.get(), (int64_t)len, off, rec.pos, lead, lo, hi, counts.data());
            }
            fwrite(&rec, sizeof rec, 1, fo);
            fwrite(&rc, 4, 1, fo);
        }
        if (!counts.empty()) fwrite(counts.data(), 4, counts.size(), fo);
        std::vector<mpn_pileup_cand> rows;
        for (int64_t i = 0; i < hi - lo; ++i) {
            mpn_pileup_cand row;
            memset(&row, 0, sizeof row);
            if (!pile_decide(&counts[(size_t)i * MPN_PILEUP_SLOTS], ref[i], min_coverage, threshold, &row)) continue;
            row.pos = (int32_t)(lo + i);
            rows.push_back(row);
        }
        const uint64_t n_cand = rows.size();
        fwrite(&n_cand, 8, 1, fo);
        if (!rows.empty()) fwrite(rows.data(), sizeof(mpn_pileup_cand), rows.size(), fo);
    }
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 1;
}
