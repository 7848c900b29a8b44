// Runs the local-realignment arithmetic of megapath_nano_amd/csrc/local_realign_core.h on the CPU, serially -- membership with the
// depth rule, the rows at which the script's parser raises, the surviving columns, the fragments, the allele keys of every read and the ordered tally of a site -- so that every
// test case, malformed records included, has been through the bounds decisions under the host's tools before it meets a GPU.  SSW
// comes from oracle/ssw_oracle.c, compiled in:
//
//   gcc -O1 -g -fsanitize=address,undefined -c oracle/ssw_oracle.c -o ssw_oracle.o
//   g++ -O1 -g -fsanitize=address,undefined -o local_realign_host_check scripts/local_realign_host_check.cpp ssw_oracle.o
//   local_realign_host_check cases.bin results.bin
//
// cases.bin:   u32 n, then per case u64 text length, u64 contig length, i32 maxcnt, u32 rows, u32 sites, the text, the contig, then per
//              row i64 off, i64 pos (0-based), i64 end (exclusive): the records mpileup may take, in file order; then per site i32 pos.
// results.bin: per case, per site: i32 state (0: done; 1: the script raises; 100 + why: the row `bad` is refused), i64 bad, i32 depth,
//              u32 reads (fragments), u32 keys, then per key i32 count, u32 len and the len bytes of its text, in the order of first
//              insertion.
// The text and the contig are heap blocks of their exact size: a read outside them is reported.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../megapath_nano_amd/csrc/local_realign_core.h"

using namespace mpn_lr;

extern "C" {
typedef struct {
    uint16_t score1, score2;
    int32_t ref_begin1, ref_end1, read_begin1, read_end1, ref_end2;
    int32_t cigar_len;
    int32_t status;
} ssw_oracle_result;
int ssw_oracle_align(const int8_t *read, int32_t readLen, const int8_t *mat, int32_t n, int8_t score_size, const int8_t *ref, int32_t refLen,
                     uint8_t gapO, uint8_t gapE, uint8_t flag, uint16_t filters, int32_t filterd, int32_t maskLen, ssw_oracle_result *r,
                     uint32_t *cigar_buf, int32_t cigar_cap);
}

static bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
template <class T> static void put(FILE *f, T v) { fwrite(&v, sizeof v, 1, f); }

struct Row { int64_t off, pos, end; };
struct Frag { int64_t first; size_t row; int64_t off; int32_t len; };

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]); return 2; }
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) { perror("open"); return 2; }
    static const int8_t MAT[25] = {4, -6, -6, -6, 0, -6, 4, -6, -6, 0, -6, -6, 4, -6, 0, -6, -6, -6, 4, 0, 0, 0, 0, 0, 0};
    uint32_t n = 0;
    if (!read_exact(fi, &n, 4)) { fprintf(stderr, "short case file\n"); return 2; }
    for (uint32_t c = 0; c < n; ++c) {
        uint64_t len = 0, clen = 0;
        int32_t maxcnt = 0;
        uint32_t n_rows = 0, n_sites = 0;
        if (!read_exact(fi, &len, 8) || !read_exact(fi, &clen, 8) || !read_exact(fi, &maxcnt, 4) || !read_exact(fi, &n_rows, 4) || !read_exact(fi, &n_sites, 4)) {
            fprintf(stderr, "bad case file\n");
            return 2;
        }
        std::unique_ptr<uint8_t[]> text(new uint8_t[len]), contig(new uint8_t[clen]);
        std::vector<Row> rows(n_rows);
        std::vector<int32_t> sites(n_sites);
        if (!read_exact(fi, text.get(), len) || !read_exact(fi, contig.get(), clen) || !read_exact(fi, rows.data(), sizeof(Row) * n_rows) ||
            !read_exact(fi, sites.data(), 4 * (size_t)n_sites)) {
            fprintf(stderr, "short case file\n");
            return 2;
        }
        for (int32_t pos1 : sites) {
            // membership: htslib's overlap with the 0-based region [pos1 - 234, pos1 + 234), then the depth rule
            std::vector<size_t> cand;
            std::vector<int64_t> cs, ce;
            for (size_t r = 0; r < rows.size(); ++r)
                if (rows[r].pos < (int64_t)pos1 + REGION + 1 && rows[r].end > (int64_t)pos1 - REGION - 1) { cand.push_back(r); cs.push_back(rows[r].pos); ce.push_back(rows[r].end); }
            std::vector<uint8_t> keep(cand.size(), 1);
            if ((int64_t)cand.size() >= maxcnt) lr_depth_rule((int64_t)cand.size(), cs.data(), ce.data(), maxcnt, keep.data());
            std::vector<size_t> acc;
            for (size_t i = 0; i < cand.size(); ++i) if (keep[i]) acc.push_back(cand[i]);
            // columns
            uint32_t cov[WORDS] = {0}, bad[WORDS] = {0}, mask[WORDS];
            int why = 0;
            int64_t bad_row = -1;
            for (size_t r : acc) {
                why = rows[r].off < 0 || rows[r].off > (int64_t)len - BAMW_FIXED ? MPN_LR_PAST : lr_cover_serial(text.get(), (int64_t)len, rows[r].off, rows[r].pos, pos1, cov, bad);
                if (why) { bad_row = (int64_t)r; break; }
            }
            lr_finish_mask(cov, bad, mask);
            // fragments, in the order of the script's dict
            std::vector<Frag> frags;
            std::vector<uint8_t> letters;
            for (size_t k = 0; k < acc.size() && !why; ++k) {
                const Row &rw = rows[acc[k]];
                int64_t cnt = 0, first = 0;
                why = lr_frag_serial(text.get(), (int64_t)len, rw.off, rw.pos, pos1, mask, nullptr, &cnt, &first);
                if (why) { bad_row = (int64_t)acc[k]; break; }
                if (cnt == 0) continue;
                const size_t at = letters.size();
                letters.resize(at + (size_t)cnt);
                int64_t again = 0;
                if (lr_frag_serial(text.get(), (int64_t)len, rw.off, rw.pos, pos1, mask, letters.data() + at, &again, &first) || again != cnt) { fprintf(stderr, "the passes differ\n"); return 3; }
                frags.push_back(Frag{first, acc[k], (int64_t)at, (int32_t)cnt});
            }
            if (why) {
                put<int32_t>(fo, 100 + why); put<int64_t>(fo, bad_row); put<int32_t>(fo, 0); put<uint32_t>(fo, 0); put<uint32_t>(fo, 0);
                continue;
            }
            // the script's parser raises on a row that begins with an unknown letter and an indel behind it
            bool parser_raises = false;
            for (size_t k = 0; k < acc.size() && !parser_raises; ++k) {
                int64_t cols[64];
                const int nh = lr_hazard_serial(text.get(), (int64_t)len, rows[acc[k]].off, rows[acc[k]].pos, pos1, cols, 64);
                for (int h = 0; h < nh && !parser_raises; ++h) {
                    bool entry = false;
                    for (size_t j = 0; j < k && !entry; ++j) entry = lr_entry_at(text.get(), (int64_t)len, rows[acc[j]].off, rows[acc[j]].pos, cols[h]);
                    parser_raises = !entry;
                }
            }
            if (parser_raises) {
                put<int32_t>(fo, 1); put<int64_t>(fo, -1); put<int32_t>(fo, 0); put<uint32_t>(fo, (uint32_t)frags.size()); put<uint32_t>(fo, 0);
                continue;
            }
            std::stable_sort(frags.begin(), frags.end(), [](const Frag &a, const Frag &b) { return a.first != b.first ? a.first < b.first : a.row < b.row; });
            // the reference window and SSW
            const int64_t w_lo = (int64_t)pos1 - FLANK_REF - 1, w_hi = std::min<int64_t>((int64_t)pos1 + FLANK_REF, (int64_t)clen);
            std::vector<int8_t> window;
            for (int64_t p = w_lo; p < w_hi; ++p) window.push_back(lr_ssw_code(contig[p]));
            struct Occ { LrKeyRef key; uint64_t rank; };
            struct Ssw { int st; ssw_oracle_result res; std::vector<uint32_t> cig; };
            std::map<std::string, Ssw> done;
            std::vector<Occ> occ;
            bool raises = false;
            for (size_t j = 0; j < frags.size() && !raises; ++j) {
                const Frag &f = frags[j];
                std::vector<int8_t> codes((size_t)f.len);
                for (int32_t i = 0; i < f.len; ++i) codes[i] = lr_ssw_code(letters[(size_t)f.off + i]);
                // (equal fragments of one site have equal results: a deep pile of copies is aligned once)
                const std::string text_of(letters.begin() + f.off, letters.begin() + f.off + f.len);
                auto hit = done.find(text_of);
                if (hit == done.end()) {
                    Ssw s;
                    s.cig.resize((size_t)f.len + window.size() + 8);
                    memset(&s.res, 0, sizeof s.res);
                    s.st = ssw_oracle_align(codes.data(), f.len, MAT, 5, 2, window.data(), (int32_t)window.size(), 8, 2, 2, 0, 0, f.len <= 30 ? 15 : f.len, &s.res,
                                            s.cig.data(), (int32_t)s.cig.size());
                    hit = done.emplace(text_of, std::move(s)).first;
                }
                const int st = hit->second.st;
                const ssw_oracle_result &res = hit->second.res;
                const std::vector<uint32_t> &cig = hit->second.cig;
                const int score = st == 0 ? res.score1 : 0;
                if (score <= 0) {
                    if (j == 0) raises = true;
                    continue;
                }
                LrKeyRef keys[MAX_KEYS];
                int64_t ref_pos = 0;
                const int nk = lr_pair_keys(res.ref_begin1, res.read_begin1, res.read_end1, cig.data(), res.cigar_len, f.off, f.len, pos1, (int64_t)clen, keys, &ref_pos);
                for (int s = 0; s < nk; ++s) occ.push_back(Occ{keys[s], ((uint64_t)(uint32_t)ref_pos << 32) | ((uint64_t)j << 3) | (unsigned)s});
            }
            if (raises) {
                put<int32_t>(fo, 1); put<int64_t>(fo, -1); put<int32_t>(fo, 0); put<uint32_t>(fo, (uint32_t)frags.size()); put<uint32_t>(fo, 0);
                continue;
            }
            // the tally: distinct keys, their counts, the order of first insertion
            struct Entry { LrKeyRef key; int32_t count; uint64_t rank; };
            std::vector<Entry> tab;
            for (const Occ &o : occ) {
                size_t e = 0;
                while (e < tab.size() && !lr_key_equal(o.key, tab[e].key, letters.data(), contig.get())) ++e;
                if (e == tab.size()) tab.push_back(Entry{o.key, 1, o.rank});
                else { ++tab[e].count; tab[e].rank = std::min(tab[e].rank, o.rank); }
            }
            std::sort(tab.begin(), tab.end(), [](const Entry &a, const Entry &b) { return a.rank < b.rank; });
            int32_t depth = 0;
            for (const Entry &e : tab) {
                const uint8_t c0 = lr_key_char(e.key, 0, letters.data(), contig.get());
                if (c0 != 'I' && c0 != 'D') depth += e.count;
            }
            put<int32_t>(fo, 0); put<int64_t>(fo, -1); put<int32_t>(fo, depth); put<uint32_t>(fo, (uint32_t)frags.size()); put<uint32_t>(fo, (uint32_t)tab.size());
            for (const Entry &e : tab) {
                const int32_t kl = lr_key_strlen(e.key);
                put<int32_t>(fo, e.count); put<uint32_t>(fo, (uint32_t)kl);
                for (int32_t i = 0; i < kl; ++i) fputc(lr_key_char(e.key, i, letters.data(), contig.get()), fo);
            }
        }
    }
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 2;
}
