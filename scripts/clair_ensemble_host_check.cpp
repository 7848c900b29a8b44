// The averaging of include/mpn_ensemble.h, run serially on the host through csrc/clair_ensemble_core.h: the same arithmetic and the
// same checks of the lists as the kernel's entry.  Built with g++ -ffp-contract=off under AddressSanitizer and UBSan by
// tests/test_clair_ensemble_host.py.
//
//   clair_ensemble_host_check <case file> <result file>
//   clair_ensemble_host_check --rounding
//
// The case file (little endian): int64 n_lines, n_t, n_p, probs_f64, n_sites, n_entries, n_out; int32 tensor_row[n_lines],
// prob_row[n_lines]; int32 tensors[n_t * 1056]; float32 or float64 probs[n_p * 90]; int64 site_off[n_sites + 1]; int32
// site_lines[n_entries]; int32 out_slot[n_sites].  The result file: int64 bad_site, n_out; int32 [n_out * 1056]; float32
// [n_out * 90]; int64 micro-units [n_out * 90].
// --rounding compares ens_result with snprintf("%.6f"), strtod, (float) -- and its micro-units with the digits printed -- on every
// s / c for s in 0 .. 2 000 000 micro-units and c in {1, 2, 3, 4, 7, 100, 400} (the sum formed as the kernel forms it from c
// addends), on every exact tie j / 128 (j odd) below 8 and on both float64 neighbours of each tie, with either sign; it prints
// `<cases> <mismatches>`.
// Exit status: 0; 1 for a mismatch; 2 for a case file that does not hold what it says; 3 for lists that are refused (the message
// names what and where).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../megapath_nano_amd/csrc/clair_ensemble_core.h"

using namespace mpn_ens;

static bool take(FILE *f, void *to, size_t n) { return n == 0 || fread(to, 1, n, f) == n; }

static long long n_cases = 0, n_wrong = 0;

static void compare(double q) {
    char text[64];
    snprintf(text, sizeof text, "%.6f", q);
    const float want = (float)strtod(text, nullptr);
    int64_t micro = 0;
    const float got = ens_result(q, &micro);
    long long digits = 0;
    bool minus = false;
    for (const char *c = text; *c; ++c) {
        if (*c == '-') minus = true;
        else if (*c != '.') digits = digits * 10 + (*c - '0');
    }
    ++n_cases;
    if (memcmp(&got, &want, 4) != 0 || micro != (minus ? -digits : digits)) {
        if (n_wrong++ < 20) fprintf(stderr, "q = %.17g (%a): %s, got %.9g and %lld\n", q, q, text, (double)got, (long long)micro);
    }
}

static int rounding() {
    static const int counts[] = {1, 2, 3, 4, 7, 100, 400};
    for (int c : counts)
        for (long long s = 0; s <= 2000000; ++s) {
            // c addends of s / c micro-units, the first s % c of them one more: what quantized float32 lines add
            const long long each = s / c, more = s % c;
            double sum = ens_div((double)(each + (more > 0 ? 1 : 0)), 1.0e6);
            for (int i = 1; i < c; ++i) sum = ens_add(sum, ens_div((double)(each + (i < more ? 1 : 0)), 1.0e6));
            compare(ens_div(sum, (double)c));
        }
    for (int j = 1; j < 8 * 128; j += 2) {
        const double tie = (double)j / 128.0;
        for (double q : {tie, std::nextafter(tie, 0.0), std::nextafter(tie, 16.0)}) {
            compare(q);
            compare(-q);
        }
    }
    for (double q : {0.0, -0.0, 4.9e-324, 0.5e-6, 0.49999999999999994e-6, 1.5e-6, 2.5e-6, 1e-7, -1e-7, 7.999999499, 2147483647.9999995, 2147483647.4999995})
        compare(q);
    printf("%lld %lld\n", n_cases, n_wrong);
    return n_wrong ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && strcmp(argv[1], "--rounding") == 0) return rounding();
    if (argc != 3) { fprintf(stderr, "usage: clair_ensemble_host_check <case file> <result file> | --rounding\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int64_t head[7];
    if (!take(f, head, sizeof head)) { fprintf(stderr, "short case file\n"); return 2; }
    const int64_t n_lines = head[0], n_t = head[1], n_p = head[2], f64 = head[3], n_sites = head[4], n_entries = head[5], n_out = head[6];
    for (int i = 0; i < 7; ++i)
        if (head[i] < 0 || head[i] > (1ll << 24)) { fprintf(stderr, "a size of the case file is out of range\n"); return 2; }
    std::vector<int32_t> tensor_row((size_t)n_lines), prob_row((size_t)n_lines), tensors((size_t)n_t * CELLS), site_lines((size_t)n_entries), out_slot((size_t)n_sites);
    std::vector<float> p32(f64 ? 0 : (size_t)n_p * PROBS);
    std::vector<double> p64(f64 ? (size_t)n_p * PROBS : 0);
    std::vector<int64_t> site_off((size_t)n_sites + 1);
    if (!take(f, tensor_row.data(), tensor_row.size() * 4) || !take(f, prob_row.data(), prob_row.size() * 4) || !take(f, tensors.data(), tensors.size() * 4) ||
        !take(f, p32.data(), p32.size() * 4) || !take(f, p64.data(), p64.size() * 8) || !take(f, site_off.data(), site_off.size() * 8) ||
        !take(f, site_lines.data(), site_lines.size() * 4) || !take(f, out_slot.data(), out_slot.size() * 4)) {
        fprintf(stderr, "short case file\n");
        return 2;
    }
    fclose(f);
    if (n_out > n_sites) { fprintf(stderr, "refused: more output slots than sites\n"); return 3; }
    for (int64_t s = 0; s <= n_sites; ++s)       // the gather below walks site_off[n_sites] entries of a list of n_entries
        if (site_off[s] < 0 || site_off[s] > n_entries || (s == n_sites && n_sites > 0 && site_off[s] != n_entries)) {
            fprintf(stderr, "refused: offset %lld does not lie inside the %lld entries\n", (long long)s, (long long)n_entries);
            return 3;
        }
    std::vector<int32_t> row_t((size_t)n_entries), row_p((size_t)n_entries);
    std::vector<uint8_t> used((size_t)n_out);
    int64_t at = -1;
    const int what = ens_check_gather(n_lines, tensor_row.data(), prob_row.data(), n_t, n_p, n_sites, site_off.data(), site_lines.data(), out_slot.data(),
                                      n_out, row_t.data(), row_p.data(), used.data(), &at);
    if (what) { fprintf(stderr, "refused: %d at %lld\n", what, (long long)at); return 3; }
    std::vector<int32_t> out_t((size_t)n_out * CELLS);
    std::vector<float> out_p((size_t)n_out * PROBS);
    std::vector<int64_t> out_m((size_t)n_out * PROBS);
    int64_t bad_site = -1;
    for (int64_t s = 0; s < n_sites; ++s) {
        const int64_t slot = out_slot[s], b = site_off[s], e = site_off[s + 1];
        if (slot < 0) continue;
        for (int col = 0; col < CELLS; ++col) {
            const int64_t sum = ens_cell(tensors.data(), row_t.data(), b, e, col);
            if (sum != (int64_t)(int32_t)sum && bad_site < 0) bad_site = s;
            out_t[(size_t)slot * CELLS + col] = (int32_t)(uint32_t)(uint64_t)sum;
        }
        for (int col = 0; col < PROBS; ++col) {
            const double q = f64 ? ens_mean(p64.data(), row_p.data(), b, e, col) : ens_mean(p32.data(), row_p.data(), b, e, col);
            out_p[(size_t)slot * PROBS + col] = ens_result(q, &out_m[(size_t)slot * PROBS + col]);
        }
    }
    FILE *g = fopen(argv[2], "wb");
    if (!g) { perror(argv[2]); return 2; }
    const int64_t tail[2] = {bad_site, n_out};
    fwrite(tail, sizeof tail, 1, g);
    if (n_out > 0) {          // (an empty vector's data() may be null, which fwrite must not be given)
        fwrite(out_t.data(), 4, out_t.size(), g);
        fwrite(out_p.data(), 4, out_p.size(), g);
        fwrite(out_m.data(), 8, out_m.size(), g);
    }
    return fclose(g) == 0 ? 0 : 2;
}
