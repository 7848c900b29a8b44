// Host build of the de Bruijn graph consensus: csrc/dbg_core.h run serially, one lane per window, for tests/test_dbg_host.py (under
// AddressSanitizer and UBSan) and, at -O2, as the baseline of scripts/bench_dbg_consensus.py.
//
//   dbg_host_check run  <cases> <results>     every window of <cases>, results written to <results>
//   dbg_host_check time <cases>               the same without output; prints the milliseconds the windows took
//
// <cases>, little endian:  u32 n_windows, then per window
//   u32 slots (0: the smallest table), u32 grow (0: report a full table or buffer; 1: enlarge and redo), u32 ref_len, ref bytes,
//   u32 n_reads, per read u32 len, bases, mask bytes
// <results>: per window  i32 status, i32 k, i32 n, i32 redone, per haplotype u32 len, bytes
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../megapath_nano_amd/csrc/dbg_core.h"

struct Case {
    uint32_t slots, grow;
    std::vector<uint8_t> seq, mask;
    std::vector<uint32_t> read_off;
    uint32_t ref_len;
};

struct Result {
    int status = 0, k = 0, redone = 0;
    std::vector<std::string> haps;
};

static bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static bool load(const char *path, std::vector<Case> &cases) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint32_t n = 0;
    bool ok = read_exact(f, &n, 4);
    for (uint32_t w = 0; ok && w < n; ++w) {
        Case c;
        uint32_t n_reads = 0;
        ok = read_exact(f, &c.slots, 4) && read_exact(f, &c.grow, 4) && read_exact(f, &c.ref_len, 4);
        if (!ok) break;
        c.seq.resize(c.ref_len);
        c.mask.assign(c.ref_len, 0);
        ok = read_exact(f, c.seq.data(), c.ref_len) && read_exact(f, &n_reads, 4);
        c.read_off.push_back(c.ref_len);
        for (uint32_t r = 0; ok && r < n_reads; ++r) {
            uint32_t len = 0;
            ok = read_exact(f, &len, 4);
            if (!ok) break;
            const size_t at = c.seq.size();
            c.seq.resize(at + len);
            c.mask.resize(at + len);
            ok = read_exact(f, c.seq.data() + at, len) && read_exact(f, c.mask.data() + at, len);
            c.read_off.push_back((uint32_t)c.seq.size());
        }
        cases.push_back(std::move(c));
    }
    fclose(f);
    return ok;
}

static uint32_t pow2_at_least(uint64_t v) {
    uint32_t p = DBG_MIN_SLOTS;
    while (p < v) p <<= 1;
    return p;
}

static Result run(const Case &c) {
    Result res;
    DbgWindow win{c.seq.data(), c.mask.data(), c.read_off.data(), c.ref_len, (uint32_t)c.read_off.size() - 1, (uint32_t)c.seq.size()};
    uint32_t slots = pow2_at_least(c.slots), hap_cap = c.ref_len + 16;
    DbgShared sh;
    for (;;) {
        // every array at its exact size, so that the sanitizer sees an index that leaves it
        std::vector<uint32_t> loc(slots), succ(5 * (size_t)slots), pred(5 * (size_t)slots), w(4 * (size_t)slots), refmask(slots),
            indeg(slots), flags(slots), order(slots), refslot(c.ref_len);
        std::vector<uint8_t> rem(c.seq.size()), hap((size_t)DBG_MAXP * hap_cap);
        DbgWork wk{slots, hap_cap, loc.data(), succ.data(), pred.data(), w.data(), refmask.data(), indeg.data(), flags.data(),
                   order.data(), refslot.data(), rem.data(), hap.data()};
        memset(&sh, 0, sizeof sh);
        int k = 0, n = 0;
        res.status = dbg_window(win, wk, &sh, 0, 1, &k, &n);
        res.k = k;
        if (c.grow && res.status == DBG_TABLE_FULL) { slots *= 2; ++res.redone; continue; }
        if (c.grow && res.status == DBG_HAP_FULL) { hap_cap *= 2; ++res.redone; continue; }
        for (int i = 0; i < n; ++i)
            res.haps.emplace_back((const char *)hap.data() + (size_t)sh.out_buf[i] * hap_cap, sh.out_len[i]);
        return res;
    }
}

int main(int argc, char **argv) {
    if (argc < 3 || (strcmp(argv[1], "run") && strcmp(argv[1], "time")) || (!strcmp(argv[1], "run") && argc < 4)) {
        fprintf(stderr, "usage: %s run <cases> <results> | time <cases>\n", argv[0]);
        return 2;
    }
    std::vector<Case> cases;
    if (!load(argv[2], cases)) { fprintf(stderr, "cannot read %s\n", argv[2]); return 1; }
    if (!strcmp(argv[1], "time")) {
        const auto t0 = std::chrono::steady_clock::now();
        size_t haps = 0;
        for (const Case &c : cases) haps += run(c).haps.size();
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        printf("{\"windows\": %zu, \"haplotypes\": %zu, \"ms\": %.3f}\n", cases.size(), haps, ms);
        return 0;
    }
    FILE *out = fopen(argv[3], "wb");
    if (!out) { fprintf(stderr, "cannot write %s\n", argv[3]); return 1; }
    for (const Case &c : cases) {
        const Result r = run(c);
        const int32_t head[4] = {r.status, r.k, (int32_t)r.haps.size(), r.redone};
        fwrite(head, 4, 4, out);
        for (const std::string &h : r.haps) {
            const uint32_t len = (uint32_t)h.size();
            fwrite(&len, 4, 1, out);
            fwrite(h.data(), 1, len, out);
        }
    }
    return fclose(out) == 0 ? 0 : 1;
}
