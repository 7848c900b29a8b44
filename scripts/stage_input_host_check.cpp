// Runs megapath_nano_amd/csrc/stage_input.h, the host half of the stage-test entries' input layer, on the CPU: valid pair sets
// (one pair; three with gaps between them, one without a CIGAR, the last ending exactly where the buffers end) and every refusal
// once, with its message; the CSR offsets; and the made index, the made minimizers, the options and the knobs of
// mpn_seed_anchors_batch, each refusal once.  So the checks are checked without a GPU and under the host's tools:
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -o stage_input_host_check scripts/stage_input_host_check.cpp
//   stage_input_host_check
//
// Every input array is a heap block of its exact size: a read outside it is reported.  Exit status 1 if an expectation fails.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>

#include "../megapath_nano_amd/csrc/stage_input.h"

using namespace mpn_stage;

static std::string g_msg;
static int g_failed = 0;

static void sink(const char *fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_msg = buf;
}

static void expect(const char *what, bool ok) {
    if (!ok) { fprintf(stderr, "failed: %s (last message: '%s')\n", what, g_msg.c_str()); ++g_failed; }
}

struct Set {
    std::vector<uint8_t> qc, tc;
    std::vector<int64_t> qoff, toff, coff;
    std::vector<int32_t> qlen, tlen, qs, qe, ts, ncig;
    std::vector<uint32_t> cig;
    bool build(bool with_cigar, bool allow_empty, StagePairs &sp) const {
        g_msg.clear();
        return stage_pairs_build("mpn_x", (int32_t)qlen.size(), qc.data(), qoff.data(), qlen.data(), tc.data(), toff.data(), tlen.data(),
                                 with_cigar ? qs.data() : nullptr, with_cigar ? qe.data() : nullptr, with_cigar ? ts.data() : nullptr,
                                 with_cigar ? cig.data() : nullptr, with_cigar ? coff.data() : nullptr, with_cigar ? ncig.data() : nullptr,
                                 allow_empty, sink, sp);
    }
    void refused(const char *what, const char *msg, bool allow_empty = false) const {
        StagePairs sp;
        expect(what, !build(true, allow_empty, sp) && g_msg == msg);
    }
};

static uint32_t op(uint32_t len, uint32_t kind) { return len << 4 | kind; }

// pair 0: read [0, 10), [2, 9) aligned as 3M 1I 3M 2D from target base 1 of [0, 12); pair 1: read [14, 20), target [20, 25), no
// CIGAR (two op slots left free at 4); pair 2: read [25, 40) as 15M on target [30, 45): both end with their buffers
static Set three() {
    Set s;
    s.qc.resize(40); s.tc.resize(45);
    for (size_t i = 0; i < s.qc.size(); ++i) s.qc[i] = (uint8_t)(i % 5);
    for (size_t i = 0; i < s.tc.size(); ++i) s.tc[i] = (uint8_t)(i % 4);
    s.qc[39] = 9;   // no code: read as N
    s.qoff = {0, 14, 25}; s.qlen = {10, 6, 15}; s.toff = {0, 20, 30}; s.tlen = {12, 5, 15};
    s.qs = {2, 0, 0}; s.qe = {9, 0, 15}; s.ts = {1, 0, 0};
    s.cig = {op(3, 0), op(1, 1), op(3, 0), op(2, 2), 0, 0, op(15, 0)};
    s.coff = {0, 4, 6}; s.ncig = {4, 0, 1};
    return s;
}

static Set one() {
    Set s = three();
    s.qc.resize(10); s.tc.resize(12); s.cig.resize(4);
    for (auto *v : {&s.qoff, &s.toff, &s.coff}) v->resize(1);
    for (auto *v : {&s.qlen, &s.tlen, &s.qs, &s.qe, &s.ts, &s.ncig}) v->resize(1);
    return s;
}

static void valid_sets() {
    StagePairs sp;
    const Set s1 = one(), s3 = three();
    expect("n = 1", s1.build(true, false, sp) && sp.qtot == 10 && sp.ttot == 12 && sp.ctot == 4 && sp.reads.size() == 28 && sp.cigar.size() == 5 &&
                        sp.qspan[0] == 7 && sp.tspan[0] == 8);
    expect("n = 1 without CIGARs", s1.build(false, false, sp) && sp.qtot == 10 && sp.ttot == 12 && sp.ctot == 0 && sp.cigar.empty() && sp.qspan.empty());
    bool ok = s3.build(true, false, sp) && sp.n == 3 && sp.qtot == 40 && sp.ttot == 45 && sp.ctot == 7 && sp.reads.size() == 56 && sp.cigar.size() == 8 &&
              sp.cigar[7] == 0 && sp.qspan == std::vector<int32_t>({7, 0, 15}) && sp.tspan == std::vector<int32_t>({8, 0, 15}) && sp.tcodes == s3.tc.data();
    for (size_t i = 0; ok && i < sp.reads.size(); ++i) ok = sp.reads[i] == (i < 39 ? "ACGTN"[i % 5] : 'N');
    for (size_t i = 0; ok && i < 7; ++i) ok = sp.cigar[i] == s3.cig[i];
    expect("n = 3, gaps between the pairs, the last pair ending at qtot", ok);
}

static void refusals() {
    Set s = three();
    s.qlen[1] = -1;
    s.refused("negative length", "mpn_x: pair 1: intervals outside the sequences");
    s = three(); s.qe[0] = 11;
    s.refused("qe > q_len", "mpn_x: pair 0: intervals outside the sequences");
    s = three(); s.ts[1] = 6;
    s.refused("ts > t_len", "mpn_x: pair 1: intervals outside the sequences");
    s = three(); s.coff[1] = -1;
    s.refused("negative cig_off", "mpn_x: pair 1: intervals outside the sequences");
    s = three(); s.qoff[0] = -1;
    s.refused("negative q_off", "mpn_x: pair 0: an offset negative, or an end beyond 2^30 - 1");
    s = three(); s.toff[2] = (int64_t)1 << 40;
    s.refused("t_off far outside any buffer", "mpn_x: pair 2: an offset negative, or an end beyond 2^30 - 1");
    s = three(); s.qoff[2] = INT64_MAX;
    s.refused("q_off + q_len beyond int64", "mpn_x: pair 2: an offset negative, or an end beyond 2^30 - 1");
    s = three(); s.cig[1] = op(1, 4);
    s.refused("op > 2", "mpn_x: pair 0: op 1 is not a non-empty M, I or D");
    s.refused("op > 2, empty ops allowed", "mpn_x: pair 0: op 1 is not M, I or D", true);
    s = three(); s.ncig[1] = 1;   // (its op slot holds 0: an empty M)
    s.refused("empty op", "mpn_x: pair 1: op 0 is not a non-empty M, I or D");
    StagePairs sp;
    expect("empty op, allowed", s.build(true, true, sp) && sp.qspan[1] == 0 && sp.tspan[1] == 0);
    s = three(); s.cig[2] = op(2, 0);
    s.refused("CIGAR one base short of its read interval", "mpn_x: pair 0: the CIGAR does not consume its read interval or leaves the target");
    s = three(); s.ts[2] = 1;
    s.refused("CIGAR one base past the target", "mpn_x: pair 2: the CIGAR does not consume its read interval or leaves the target");
}

static void csr() {
    const std::vector<int64_t> good = {0, 0, 5, 5 + STAGE_MAX}, first = {1, 2, 3, 4}, down = {0, 4, 3, 5}, wide = {0, 1, 1 + 0x40000000ll, 1 + 0x40000000ll};
    g_msg.clear();
    expect("CSR offsets", stage_csr_ok("mpn_x", 3, good.data(), sink) && g_msg.empty());
    expect("no reads", stage_csr_ok("mpn_x", 0, nullptr, sink));
    expect("a first offset != 0", !stage_csr_ok("mpn_x", 3, first.data(), sink) && g_msg == "mpn_x: offsets do not start at 0");
    expect("a decreasing offset", !stage_csr_ok("mpn_x", 3, down.data(), sink) && g_msg == "mpn_x: read 1: offsets out of order");
    expect("a row of 0x40000000", !stage_csr_ok("mpn_x", 3, wide.data(), sink) && g_msg == "mpn_x: read 1: offsets out of order");
}

// mpn_seed_anchors_batch: an index of two targets (100 and 50 bases), three keys with 2, 1 and 3 positions at k = 4 (hashes below 256);
// two reads of 3 and 0 minimizers, then one of 2
struct Seed {
    static uint64_t w(uint64_t rid, uint64_t p, uint64_t strand) { return rid << 32 | p << 1 | strand; }
    static uint64_t m(uint64_t hash, uint64_t span) { return hash << 8 | span; }
    std::vector<int32_t> lens = {100, 50}, seq_len = {60, 0, 40};
    std::vector<uint64_t> keys = {3, 77, 255};
    std::vector<int64_t> key_off = {0, 2, 3, 6}, mz_off = {0, 3, 3, 5};
    std::vector<uint64_t> pos = {w(0, 5, 0), w(1, 49, 1), w(0, 99, 0), w(0, 0, 1), w(1, 0, 0), w(1, 7, 1)};
    // x of the minimizers; their last positions 3, 20, 59 | | 39, 39 (the first spans its read from base 0, the fourth all 40 bases)
    std::vector<uint64_t> mz = {m(3, 4), m(255, 10), m(9, 1), m(0, 40), m(77, 2)}, last = {3, 20, 59, 39, 39}, strand = {0, 1, 0, 1, 0};
    bool index(int32_t k = 4) const {
        g_msg.clear();
        return stage_seed_index_ok("mpn_x", k, (int32_t)lens.size(), lens.data(), (int64_t)keys.size(), keys.data(), key_off.data(), pos.data(), sink);
    }
    bool reads() const {
        std::vector<uint64_t> xy;   // (x, y) pairs in a block of their exact size
        for (size_t i = 0; i < mz.size(); ++i) { xy.push_back(mz[i]); xy.push_back((uint64_t)(i < 3 ? 0 : 2) << 32 | last[i] << 1 | strand[i]); }
        xy.shrink_to_fit();
        g_msg.clear();
        return stage_seed_mz_ok("mpn_x", 4, (int32_t)seq_len.size(), mz_off.data(), xy.data(), seq_len.data(), sink);
    }
};

static void seed_inputs() {
    Seed s;
    expect("seed index", s.index() && g_msg.empty());
    expect("seed minimizers", s.reads() && g_msg.empty());
    expect("no reads", stage_seed_mz_ok("mpn_x", 4, 0, nullptr, nullptr, nullptr, sink));
    {
        const int32_t one = 10;
        const int64_t zero = 0;
        g_msg.clear();
        expect("an index without keys", stage_seed_index_ok("mpn_x", 15, 1, &one, 0, nullptr, &zero, nullptr, sink) && g_msg.empty());
    }
    const char *shape = "mpn_x: index: k outside 1 .. 28, no target, a key count outside 0 .. 2^30 - 1 or an array missing";
    expect("k = 0", !s.index(0) && g_msg == shape);
    expect("k = 29", !s.index(29) && g_msg == shape);
    s = Seed(); s.lens[1] = -1;
    expect("negative target length", !s.index() && g_msg == "mpn_x: index: target 1: negative length");
    s = Seed(); s.key_off[0] = 1;
    expect("key offsets from 1", !s.index() && g_msg == "mpn_x: offsets do not start at 0");
    s = Seed(); s.key_off[2] = 1;
    expect("key offsets decrease", !s.index() && g_msg == "mpn_x: read 1: offsets out of order");
    s = Seed(); s.keys[1] = 3;
    expect("equal keys", !s.index() && g_msg == "mpn_x: index: key 1: not ascending, or outside 2k bits");
    s = Seed(); s.keys[2] = 256;
    expect("a key of 2k + 1 bits", !s.index() && g_msg == "mpn_x: index: key 2: not ascending, or outside 2k bits");
    s = Seed(); s.pos[1] = Seed::w(2, 0, 0);
    expect("rid = n_seq", !s.index() && g_msg == "mpn_x: index: position 1: outside its target");
    s = Seed(); s.pos[5] = Seed::w(1, 50, 1);
    expect("position = the target's length", !s.index() && g_msg == "mpn_x: index: position 5: outside its target");
    s = Seed(); s.pos[0] = Seed::w(0x7fffffff, 0, 0) | 1ull << 63;
    expect("rid of 32 bits", !s.index() && g_msg == "mpn_x: index: position 0: outside its target");

    s = Seed(); s.mz_off[1] = 6;
    expect("minimizer offsets decrease", !s.reads() && g_msg == "mpn_x: read 1: offsets out of order");
    s = Seed(); s.seq_len[1] = -1;
    expect("negative read length", !s.reads() && g_msg == "mpn_x: read 1: negative length");
    s = Seed(); s.mz[1] = (uint64_t)256 << 8 | 10;
    expect("hash of 2k + 1 bits", !s.reads() && g_msg == "mpn_x: read 0: minimizer 1: hash outside 2k bits");
    s = Seed(); s.mz[0] = (uint64_t)3 << 8;
    expect("span 0", !s.reads() && g_msg == "mpn_x: read 0: minimizer 0: span outside 1 .. min(255, last_pos + 1)");
    s = Seed(); s.mz[0] = (uint64_t)3 << 8 | 5;
    expect("span = last_pos + 2", !s.reads() && g_msg == "mpn_x: read 0: minimizer 0: span outside 1 .. min(255, last_pos + 1)");
    s = Seed(); s.last[2] = 60;
    expect("last_pos = seq_len", !s.reads() && g_msg == "mpn_x: read 0: minimizer 2: last_pos outside the read");
    s = Seed(); s.last[4] = 38;
    expect("last_pos decreases", !s.reads() && g_msg == "mpn_x: read 2: minimizer 1: last_pos decreases");
    s = Seed(); s.last[3] = 0x7fffffff;
    expect("last_pos of 31 bits", !s.reads() && g_msg == "mpn_x: read 2: minimizer 0: last_pos outside the read");

    g_msg.clear();
    expect("knobs", stage_seed_knobs_ok("mpn_x", 1, 0, 0, 0, 0, 0, 0, sink) && stage_seed_knobs_ok("mpn_x", 1 << 25, 5, 66076418, INT64_MAX, 3, 1, 9, sink) && g_msg.empty());
    expect("mid_occ 0", !stage_seed_knobs_ok("mpn_x", 0, 3, 5000, 0, 0, 0, 0, sink) && g_msg == "mpn_x: mid_occ 0 outside 1 .. 2^25");
    expect("mid_occ 2^25 + 1", !stage_seed_knobs_ok("mpn_x", (1 << 25) + 1, 3, 5000, 0, 0, 0, 0, sink) && g_msg == "mpn_x: mid_occ 33554433 outside 1 .. 2^25");
    expect("min_cnt -1", !stage_seed_knobs_ok("mpn_x", 9, -1, 5000, 0, 0, 0, 0, sink) && g_msg == "mpn_x: a negative option");
    expect("max_gap -1", !stage_seed_knobs_ok("mpn_x", 9, 3, -1, 0, 0, 0, 0, sink) && g_msg == "mpn_x: a negative option");
    const char *knob = "mpn_x: flt_round2, flt_wgs, grid_cap or the capacity negative";
    expect("flt_round2 -1", !stage_seed_knobs_ok("mpn_x", 9, 3, 5000, -1, 0, 0, 0, sink) && g_msg == knob);
    expect("flt_wgs -1", !stage_seed_knobs_ok("mpn_x", 9, 3, 5000, 0, -1, 0, 0, sink) && g_msg == knob);
    expect("grid_cap -1", !stage_seed_knobs_ok("mpn_x", 9, 3, 5000, 0, 0, -1, 0, sink) && g_msg == knob);
    expect("cap -1", !stage_seed_knobs_ok("mpn_x", 9, 3, 5000, 0, 0, 0, -1, sink) && g_msg == knob);
}

int main() {
    valid_sets();
    refusals();
    csr();
    seed_inputs();
    if (!g_failed) printf("stage_input: all expectations hold\n");
    return g_failed ? 1 : 0;
}
