// Runs BAM texts through the walk of megapath_nano_amd/csrc/bam_walk_core.h on the CPU -- the code bam_walk_kernel runs, the chain
// and the rows on one thread -- so that every test case, malformed ones included, has been through the bounds decisions under the
// host's tools before it meets a GPU:
//
//   g++ -O1 -g -fsanitize=address,undefined -o bam_walk_host_check scripts/bam_walk_host_check.cpp
//   bam_walk_host_check cases.bin results.bin
//
// cases.bin:   u32 n, then per case u64 text length, u64 cut (0 = none), u32 max_records per call, the text.
// results.bin: per case i32 status, u32 calls, u64 records, u64 next, then per record i64 off, i32 l_seq, u16 flag, u8 l_read_name,
//              u8 has_qual, i64 offset of the packed bases.
// A case is walked the way ingest.py walks a file: calls of max_records until one returns fewer or a status; with a cut, first
// text[0 .. cut) with final = 0 and then the unconsumed tail + text[cut ..) with final = 1, offsets counted in the whole text.
// Every text a call sees is a heap block of its exact size: a read outside it is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../megapath_nano_amd/csrc/bam_walk_core.h"

using namespace mpn_bamw;

static bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

struct Out {
    int32_t status = 0;
    uint32_t calls = 0;
    int64_t next = 0;
    std::vector<mpn_bam_row> rows;
    std::vector<int64_t> seq;
    bool at_header = true;
};

// one text (the bytes [base, base + len) of the case), walked to its end; returns the bytes consumed
static int64_t walk_text(const uint8_t *whole, int64_t base, int64_t len, bool final_call, uint32_t max_records, Out &o) {
    std::unique_ptr<uint8_t[]> t(new uint8_t[len]);
    memcpy(t.get(), whole + base, (size_t)len);
    std::unique_ptr<mpn_bam_row[]> rows(new mpn_bam_row[max_records]);
    int64_t start = 0;
    for (;;) {
        int64_t n = 0, next = 0;
        bamw_walk_serial(t.get(), len, start, o.at_header, final_call, max_records, rows.get(), &n, &next, &o.status);
        ++o.calls;
        if (o.at_header && next > start) o.at_header = false;
        for (int64_t r = 0; r < n; ++r) {
            o.seq.push_back(base + bamw_seq_off(t.get(), &rows[r]));
            rows[r].off += base;
            o.rows.push_back(rows[r]);
        }
        start = next;
        if (o.status != MPN_INFLATE_OK || n < (int64_t)max_records) break;
    }
    o.next = base + start;
    return start;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]); return 2; }
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) { perror("open"); return 2; }
    uint32_t n = 0;
    if (!read_exact(fi, &n, 4)) { fprintf(stderr, "short case file\n"); return 2; }
    for (uint32_t c = 0; c < n; ++c) {
        uint64_t len = 0, cut = 0;
        uint32_t max_records = 0;
        if (!read_exact(fi, &len, 8) || !read_exact(fi, &cut, 8) || !read_exact(fi, &max_records, 4) || max_records == 0 || cut > len) {
            fprintf(stderr, "bad case file\n");
            return 2;
        }
        std::unique_ptr<uint8_t[]> text(new uint8_t[len]);
        if (!read_exact(fi, text.get(), len)) { fprintf(stderr, "short case file\n"); return 2; }
        Out o;
        int64_t used = 0;
        if (cut) used = walk_text(text.get(), 0, (int64_t)cut, false, max_records, o);
        if (o.status == MPN_INFLATE_OK) walk_text(text.get(), used, (int64_t)len - used, true, max_records, o);
        const uint64_t records = o.rows.size();
        fwrite(&o.status, 4, 1, fo);
        fwrite(&o.calls, 4, 1, fo);
        fwrite(&records, 8, 1, fo);
        fwrite(&o.next, 8, 1, fo);
        for (size_t r = 0; r < o.rows.size(); ++r) {
            fwrite(&o.rows[r], sizeof(mpn_bam_row), 1, fo);
            fwrite(&o.seq[r], 8, 1, fo);
        }
    }
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 1;
}
