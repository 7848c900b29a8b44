// The events and the decoding of include/mpn_call.h, run serially on the host through csrc/clair_call_core.h: the same arithmetic
// and index maps as the kernels, one lane (CallSerial).  Built with g++ under AddressSanitizer and UBSan by
// tests/test_clair_call_host.py, which gives it the cases of the restatement and malformed input.
//
//   clair_call_host_check <case file>
//
// The case file (little endian): int64 text_len, n_reads, m, contig_len, options; the text; n_reads mpn_call_read; the contig; then
// per site: int32 site, int32 ref_n, int64 begin, int64 end, 33 bytes of reference string, 1056 int32, 90 float32.
// It prints, per site, `E site kind len count rank clip bases` per event and `R site status flags genotype gt21 task p-bits
// supported depth REF ALT1 ALT2` (`-` for an empty allele or key, `!` for a key that is too long); `B site read` for a bad read, `O site` for too many events.
// Exit status: 0; 2 for a case file that does not hold what it says.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../megapath_nano_amd/csrc/clair_call_core.h"

using namespace mpn_call;

static bool take(FILE *f, void *to, size_t n) { return n == 0 || fread(to, 1, n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: clair_call_host_check <case file>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int64_t head[5];
    if (!take(f, head, sizeof head)) { fprintf(stderr, "short case file\n"); return 2; }
    const int64_t text_len = head[0], n_reads = head[1], m = head[2], contig_len = head[3];
    const int32_t options = (int32_t)head[4];
    if (text_len < 0 || n_reads < 0 || m < 0 || contig_len < 0 || text_len > (1ll << 30) || n_reads > (1ll << 24) || m > (1ll << 20) || contig_len > (1ll << 30)) {
        fprintf(stderr, "a size of the case file is out of range\n");
        return 2;
    }
    std::vector<uint8_t> text((size_t)text_len), contig((size_t)contig_len);
    std::vector<mpn_call_read> reads((size_t)n_reads);
    if (!take(f, text.data(), text.size()) || !take(f, reads.data(), reads.size() * sizeof(mpn_call_read)) || !take(f, contig.data(), contig.size())) {
        fprintf(stderr, "short case file\n");
        return 2;
    }
    for (const mpn_call_read &r : reads)
        if (r.off < 0 || r.off > text_len - mpn_bamw::BAMW_FIXED || r.rlen < 0 || r.pos < 0) { fprintf(stderr, "a read outside the text\n"); return 2; }
    std::vector<mpn_call_event> ev(MPN_CALL_MAX_EVENTS);
    std::vector<uint8_t> bases((size_t)MPN_CALL_MAX_EVENTS * MAXLEN);
    CallWork *W = new CallWork;
    for (int64_t c = 0; c < m; ++c) {
        int32_t site_n[2];
        int64_t range[2];
        uint8_t ref[MPN_CALL_REF];
        std::vector<int32_t> x(CELLS);
        float probs[MPN_CALL_PROBS];
        if (!take(f, site_n, sizeof site_n) || !take(f, range, sizeof range) || !take(f, ref, sizeof ref) || !take(f, x.data(), CELLS * 4) ||
            !take(f, probs, sizeof probs)) {
            fprintf(stderr, "short case file\n");
            return 2;
        }
        if (site_n[0] < 1 || site_n[1] <= FLANK || site_n[1] > MPN_CALL_REF || range[0] < 0 || range[1] < range[0] || range[1] > n_reads) {
            fprintf(stderr, "site %lld: bad arguments\n", (long long)c);
            return 2;
        }
        int32_t n_ev = 0;
        int64_t bad = -1;
        const int rc = call_site_serial(text.data(), text_len, reads.data(), range[0], range[1], site_n[0], contig_len, ev.data(), bases.data(),
                                        MPN_CALL_MAX_EVENTS, &n_ev, &bad);
        if (rc == 1) { printf("B %d %lld\n", site_n[0], (long long)bad); continue; }
        if (rc == 2) { printf("O %d\n", site_n[0]); continue; }
        for (int32_t e = 0; e < n_ev; ++e) {
            char b[MAXLEN + 1];
            const int n = ev[e].kind == MPN_CALL_INSERTION && ev[e].key_len > 0 ? ev[e].key_len : 0;
            memcpy(b, bases.data() + (size_t)e * MAXLEN, (size_t)n);
            b[n] = 0;
            printf("E %d %d %d %d %d %d %s\n", site_n[0], ev[e].kind, ev[e].len, ev[e].count, ev[e].rank, ev[e].clip, n ? b : ev[e].key_len < 0 ? "!" : "-");
        }
        const CallSite S{probs, x.data(), ref, site_n[1], contig.data(), contig_len, (int64_t)site_n[0], ev.data(), bases.data(), n_ev, options};
        mpn_call_row row;
        memset(&row, 0, sizeof row);
        const CallSerial par;
        const int st = call_decode(par, S, W, &row);
        if (st != MPN_CALL_EMITTED) { printf("R %d %d\n", site_n[0], st); continue; }
        uint32_t bits;
        memcpy(&bits, &row.p, 4);
        auto allele = [&](int at, int n) {
            if (n == 0) { printf(" -"); return; }
            printf(" %.*s", n, (const char *)W->alleles + at);
        };
        printf("R %d %d %d %d %d %d %u %d %d", site_n[0], st, row.flags, row.genotype, row.gt21, row.genotype_task, bits, row.supported, row.depth);
        allele(0, row.ref_len);
        allele(MPN_CALL_ALT1_AT, row.alt1_len);
        allele(MPN_CALL_ALT2_AT, row.alt2_len);
        printf("\n");
    }
    delete W;
    fclose(f);
    return 0;
}
