// Runs megapath_nano_amd/csrc/read_realign_core.h on the CPU, serially -- the record arithmetic rr_records_kernel runs, the chunk
// recurrence, the counts a wave of rr_support_kernel computes, the choice rr_assign_kernel makes -- so that every test case,
// malformed records included, has been through the bounds decisions under the host's tools before it meets a GPU:
//
//   g++ -O1 -g -fsanitize=address,undefined -o read_realign_host_check scripts/read_realign_host_check.cpp
//   read_realign_host_check cases.bin results.bin
//
// cases.bin:   u32 n, then per case u64 text length, u64 contig length, i32 min_mq, u32 rows, the text, the (upper-cased) contig, per
//              row i64 off (the records of the contig in file order); then u32 reads, u32 splits, i32 pos[reads], i32 end[reads],
//              i32 win_begin[splits + 1], i32 win_start[], i32 win_end[].
// results.bin: per case, per row the 64 bytes of mpn_rr_rec (status 255: the row's fixed bytes do not lie inside the text) and i32 rc
//              of rr_support_serial on a row of its own around the record's position, whatever its status (-1: not run); then u32
//              viewed and per viewed record i32 row, i32 chunk_of, i32 taken, i32 counted; then u32 epochs and per epoch i32
//              chunk_start, i32 records that returned 1, and the 5041 counters; then per split, per read, i32 its window or -1.
// The records with MAPQ >= min_mq (if that is positive) and a position >= 0 are viewed; of those the ones with a CIGAR that pass
// the soft-clip test are taken; the taken ones with status 0 are counted (MAPQ is tested by rr_support_serial itself).  The text
// and the contig are heap blocks of their exact size: a read outside them is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../megapath_nano_amd/csrc/read_realign_core.h"

using namespace mpn_rr;

static bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static int fail(const char *what) { fprintf(stderr, "%s\n", what); return 2; }

int main(int argc, char **argv) {
    static_assert(sizeof(mpn_rr_rec) == 64, "the layout of the result file");
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]); return 2; }
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) { perror("open"); return 2; }
    uint32_t n_cases = 0;
    if (!read_exact(fi, &n_cases, 4)) return fail("short case file");
    for (uint32_t c = 0; c < n_cases; ++c) {
        uint64_t len = 0, contig_len = 0;
        int32_t min_mq = 0;
        uint32_t n_rows = 0;
        if (!read_exact(fi, &len, 8) || !read_exact(fi, &contig_len, 8) || !read_exact(fi, &min_mq, 4) || !read_exact(fi, &n_rows, 4) ||
            len > (1ull << 30) || contig_len > (1ull << 30) || n_rows > (1u << 24))
            return fail("bad case file");
        std::unique_ptr<uint8_t[]> text(new uint8_t[len]), contig(new uint8_t[contig_len]);
        std::vector<int64_t> offs(n_rows);
        if (!read_exact(fi, text.get(), len) || !read_exact(fi, contig.get(), contig_len) || !read_exact(fi, offs.data(), 8 * (size_t)n_rows))
            return fail("short case file");
        std::vector<mpn_rr_rec> recs(n_rows);
        std::vector<int32_t> viewed;
        for (uint32_t r = 0; r < n_rows; ++r) {
            mpn_rr_rec &rec = recs[r];
            memset(&rec, 0, sizeof rec);
            int32_t rc = -1;
            if (offs[r] < 0 || offs[r] > (int64_t)len - BAMW_FIXED) {
                rec.status = 255;
            } else {
                rr_record(text.get(), (int64_t)len, offs[r], &rec);
                std::vector<int32_t> own(RR_ROW, 0);
                rc = rr_support_serial(text.get(), (int64_t)len, offs[r], rec.pos, rec.pos, contig.get(), (int64_t)contig_len, (int64_t)rec.pos - 100, own.data());
                if (rec.pos >= 0 && !(min_mq > 0 && rec.mapq < min_mq)) viewed.push_back((int32_t)r);
            }
            fwrite(&rec, sizeof rec, 1, fo);
            fwrite(&rc, 4, 1, fo);
        }
        // the recurrence, and who is taken and counted
        std::vector<int32_t> pos(viewed.size()), chunk_of(viewed.size());
        for (size_t i = 0; i < viewed.size(); ++i) pos[i] = recs[viewed[i]].pos;
        int64_t first = -1, chunk = 0;
        rr_chunks_serial((int64_t)viewed.size(), pos.data(), &first, &chunk, chunk_of.data());
        const uint32_t n_viewed = (uint32_t)viewed.size();
        fwrite(&n_viewed, 4, 1, fo);
        std::vector<int32_t> counted(viewed.size(), 0);
        for (size_t i = 0; i < viewed.size(); ++i) {
            const mpn_rr_rec &rec = recs[viewed[i]];
            const int32_t taken = rec.n_cigar > 0 && rec.status != MPN_RR_PAST && rec.status != MPN_RR_BAD_OP && rec.status != MPN_RR_PLACEHOLDER &&
                                  !rec.clipped;
            counted[i] = taken && rec.status == MPN_RR_OK;
            const int32_t quad[4] = {viewed[i], chunk_of[i], taken, counted[i]};
            fwrite(quad, 4, 4, fo);
        }
        // one row per yield: the records parsed before it
        const uint32_t n_epochs = viewed.empty() ? 0 : (uint32_t)chunk + 1;
        fwrite(&n_epochs, 4, 1, fo);
        for (uint32_t k = 0; k < n_epochs; ++k) {
            const int32_t chunk_start = (int32_t)(first + (int64_t)RR_CHUNK * k);
            int32_t n_bad = 0;
            std::vector<int32_t> row(RR_ROW, 0);
            for (size_t i = 0; i < viewed.size() && chunk_of[i] <= (int32_t)k; ++i)
                if (counted[i])
                    n_bad += rr_support_serial(text.get(), (int64_t)len, offs[viewed[i]], pos[i], first + (int64_t)RR_CHUNK * chunk_of[i], contig.get(),
                                               (int64_t)contig_len, (int64_t)chunk_start - RR_EXPAND - 1, row.data());
            fwrite(&chunk_start, 4, 1, fo);
            fwrite(&n_bad, 4, 1, fo);
            fwrite(row.data(), 4, row.size(), fo);
        }
        // the assignment
        uint32_t n_reads = 0, n_splits = 0;
        if (!read_exact(fi, &n_reads, 4) || !read_exact(fi, &n_splits, 4) || n_reads > (1u << 24) || n_splits > 4096) return fail("bad case file");
        std::vector<int32_t> rpos(n_reads), rend(n_reads), begin(n_splits + 1, 0);
        if (!read_exact(fi, rpos.data(), 4 * (size_t)n_reads) || !read_exact(fi, rend.data(), 4 * (size_t)n_reads) ||
            !read_exact(fi, begin.data(), 4 * (size_t)(n_splits + 1)))
            return fail("short case file");
        for (uint32_t s = 0; s < n_splits; ++s)
            if (begin[s + 1] < begin[s] || begin[0] != 0 || begin[s + 1] > (1 << 20)) return fail("bad case file");
        const size_t n_win = (size_t)begin[n_splits];
        std::vector<int32_t> ws(n_win), we(n_win);
        if (!read_exact(fi, ws.data(), 4 * n_win) || !read_exact(fi, we.data(), 4 * n_win)) return fail("short case file");
        for (uint32_t s = 0; s < n_splits; ++s)
            for (uint32_t r = 0; r < n_reads; ++r) {
                const int32_t w = rr_assign_one(rpos[r], rend[r], begin[s + 1] - begin[s], ws.data() + begin[s], we.data() + begin[s]);
                fwrite(&w, 4, 1, fo);
            }
    }
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 1;
}
