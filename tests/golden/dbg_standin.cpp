// A host shared library that stands in for the reference's realign/debruijn_graph when tests/golden/make_read_realign_golden.py
// runs the unmodified realign_illumina_reads.py: it exports get_consensus with the script's arguments and struct, and computes the
// consensus with this project's own rule, csrc/dbg_core.h, as run() of scripts/dbg_host_check.cpp does (tables enlarged until they
// hold the window).  The reference's library needs Boost and does not compile without it.
//
//   g++ -O2 -fPIC -shared -o debruijn_graph tests/golden/dbg_standin.cpp
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../megapath_nano_amd/csrc/dbg_core.h"

struct StrArr {
    int consensus_size;
    char *consensus[500];
};

static std::vector<std::string> split(const char *s, char sep, int n) {
    std::vector<std::string> out;
    if (n <= 0) return out;
    std::string cur;
    for (const char *p = s; *p; ++p) {
        if (*p == sep) { out.push_back(cur); cur.clear(); } else cur.push_back(*p);
    }
    out.push_back(cur);
    out.resize((size_t)n);
    return out;
}

static uint32_t pow2_at_least(uint64_t v) {
    uint32_t p = DBG_MIN_SLOTS;
    while (p < v) p <<= 1;
    return p;
}

extern "C" StrArr *get_consensus(const char *ref, const char *reads, const char *low_quality, int n_reads) {
    const std::vector<std::string> seqs = split(reads, ',', n_reads), lows = split(low_quality, ',', n_reads);
    const uint32_t ref_len = (uint32_t)strlen(ref);
    std::vector<uint8_t> seq(ref, ref + ref_len), mask(ref_len, 0);
    std::vector<uint32_t> read_off{ref_len};
    for (int r = 0; r < n_reads; ++r) {
        const size_t at = seq.size();
        seq.insert(seq.end(), seqs[r].begin(), seqs[r].end());
        mask.resize(seq.size(), 0);
        const char *p = lows[r].c_str();
        while (*p) {
            char *end = nullptr;
            const long x = strtol(p, &end, 10);
            if (end == p) break;
            if (x >= 0 && (size_t)x < seqs[r].size()) mask[at + (size_t)x] = 1;
            p = end;
        }
        read_off.push_back((uint32_t)seq.size());
    }
    StrArr *res = (StrArr *)calloc(1, sizeof(StrArr));
    DbgWindow win{seq.data(), mask.data(), read_off.data(), ref_len, (uint32_t)read_off.size() - 1, (uint32_t)seq.size()};
    uint32_t slots = pow2_at_least(0), hap_cap = ref_len + 16;
    DbgShared sh;
    for (;;) {
        std::vector<uint32_t> loc(slots), succ(5 * (size_t)slots), pred(5 * (size_t)slots), w(4 * (size_t)slots), refmask(slots), indeg(slots),
            flags(slots), order(slots), refslot(ref_len);
        std::vector<uint8_t> rem(seq.size()), hap((size_t)DBG_MAXP * hap_cap);
        DbgWork wk{slots, hap_cap, loc.data(), succ.data(), pred.data(), w.data(), refmask.data(), indeg.data(), flags.data(), order.data(),
                   refslot.data(), rem.data(), hap.data()};
        memset(&sh, 0, sizeof sh);
        int k = 0, n = 0;
        const int status = dbg_window(win, wk, &sh, 0, 1, &k, &n);
        if (status == DBG_TABLE_FULL) { slots *= 2; continue; }
        if (status == DBG_HAP_FULL) { hap_cap *= 2; continue; }
        for (int i = 0; i < n && i < 500; ++i) {
            const uint32_t len = sh.out_len[i];
            char *s = (char *)malloc(len + 1);
            memcpy(s, hap.data() + (size_t)sh.out_buf[i] * hap_cap, len);
            s[len] = 0;
            res->consensus[res->consensus_size++] = s;
        }
        return res;
    }
}
