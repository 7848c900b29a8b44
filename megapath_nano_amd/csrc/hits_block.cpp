// The accumulator of a batch's hits over index parts (mpn_hits, hit_host.h): its small entries, and the hits of a range of reads
// as a byte block (index parts sharded over ranks: DESIGN section 7).
// Little-endian block: HitsBlockHead, then per read rep_len, n_hits (int32) and per hit the HIT_FIELDS int32 fields below, followed,
// when want_text, by n_cigar and the CIGAR words.  Only what merge_regs and emit_batch read travels: the hit's coordinates, scores
// and flags; everything merge_regs recomputes (id, parent, subsc, n_sub, dp_max2, mapq, sam_pri) and the transient bookkeeping of
// the mapping pass (fin_*, fx/fy/lx/ly, src, seg, as, aligned) stay behind.
#include "hit_host.h"

#include <algorithm>
#include <string.h>

using namespace mpn;

extern "C" mpn_hits *mpn_hits_create(int32_t n_reads) {
    if (n_reads < 0) { set_error("mpn_hits_create: negative read count"); return nullptr; }
    mpn_hits *h = new mpn_hits();
    h->n_reads = n_reads;
    h->regs.resize((size_t)n_reads);
    h->rep_len.assign((size_t)n_reads, 0);
    return h;
}
extern "C" void mpn_hits_destroy(mpn_hits *h) { delete h; }
extern "C" void mpn_hits_set_text(mpn_hits *h, int32_t want_text) { if (h) h->want_text = want_text ? 1 : 0; }
extern "C" int32_t mpn_hits_n_seq(const mpn_hits *h) { return (int32_t)h->lens.size(); }
extern "C" int32_t mpn_hits_n_parts(const mpn_hits *h) { return h->n_parts; }
extern "C" int32_t mpn_hits_seq_len(const mpn_hits *h, int32_t i) { return i >= 0 && (size_t)i < h->lens.size() ? h->lens[(size_t)i] : -1; }
extern "C" int32_t mpn_hits_seq_name(const mpn_hits *h, int32_t i, char *buf, int32_t cap) {
    if (i < 0 || (size_t)i >= h->names.size() || !buf || cap <= 0) return -1;
    const std::string &nm = h->names[(size_t)i];
    const int32_t l = (int32_t)std::min<size_t>(nm.size(), (size_t)cap - 1);
    memcpy(buf, nm.data(), (size_t)l);
    buf[l] = 0;
    return (int32_t)nm.size();
}

struct HitsBlockHead {
    char magic[4];
    uint32_t version;
    int32_t k, want_text, n_reads, n_seq, n_parts, pad;
    int64_t payload;      // bytes after the header
    uint64_t check;       // hits_check() of the payload
};
static const char HITS_MAGIC[4] = {'M', 'P', 'H', 'B'};
static const uint32_t HITS_VERSION = 1;
static const int HIT_FIELDS = 18;

static uint64_t hits_check(const uint8_t *p, int64_t n) {
    uint64_t h = 0x9e3779b97f4a7c15ULL ^ (uint64_t)n;
    int64_t i = 0;
    for (; i + 8 <= n; i += 8) { uint64_t w; memcpy(&w, p + i, 8); h = (h ^ w) * 0x100000001b3ULL; h ^= h >> 29; }
    for (; i < n; ++i) h = (h ^ p[i]) * 0x100000001b3ULL;
    return h;
}

static inline void hit_fields(const Reg &r, int32_t *f) {
    const int32_t v[HIT_FIELDS] = {r.cnt, r.rid, r.score, r.score0, r.qs, r.qe, r.rs, r.re, r.mlen, r.blen, (int32_t)r.rev, (int32_t)r.inv,
                                   (int32_t)r.split, (int32_t)r.hash, r.has_p, r.dp_score, r.dp_max, r.n_ambi};
    memcpy(f, v, sizeof(v));
}

static inline void hit_from_fields(const int32_t *f, Reg &r) {
    r = Reg();
    r.cnt = f[0]; r.rid = f[1]; r.score = f[2]; r.score0 = f[3]; r.qs = f[4]; r.qe = f[5]; r.rs = f[6]; r.re = f[7]; r.mlen = f[8]; r.blen = f[9];
    r.rev = (uint32_t)f[10]; r.inv = (uint32_t)f[11]; r.split = (uint32_t)f[12]; r.hash = (uint32_t)f[13]; r.has_p = f[14]; r.dp_score = f[15];
    r.dp_max = f[16]; r.n_ambi = f[17];
    r.aligned = 1;
}

extern "C" int64_t mpn_hits_export(const mpn_hits *h, int32_t lo, int32_t hi, void *buf, int64_t cap) {
    if (!h || lo < 0 || hi < lo || hi > h->n_reads) { set_error("mpn_hits_export: no accumulator or reads [%d, %d) outside its batch", lo, hi); return -1; }
    if (h->tags) { set_error("mpn_hits_export: the hits carry cs/MD strings or =/X CIGARs (out_tags 0x%x), which the block format does not hold", h->tags); return -1; }
    int64_t payload = 0;
    for (int32_t i = lo; i < hi; ++i) {
        payload += 8;
        for (const Reg &r : h->regs[(size_t)i]) payload += 4 * HIT_FIELDS + (h->want_text ? 4 + 4 * (int64_t)r.cigar.size() : 0);
    }
    const int64_t need = (int64_t)sizeof(HitsBlockHead) + payload;
    if (!buf) return need;
    if (cap < need) return -3;
    uint8_t *const base = (uint8_t *)buf, *p = base + sizeof(HitsBlockHead);
    auto put = [&](const void *src, size_t bytes) { memcpy(p, src, bytes); p += bytes; };
    int32_t f[HIT_FIELDS];
    for (int32_t i = lo; i < hi; ++i) {
        const std::vector<Reg> &regs = h->regs[(size_t)i];
        const int32_t rh[2] = {h->rep_len[(size_t)i], (int32_t)regs.size()};
        put(rh, 8);
        for (const Reg &r : regs) {
            hit_fields(r, f);
            put(f, sizeof(f));
            if (h->want_text) {
                const int32_t nc = (int32_t)r.cigar.size();
                put(&nc, 4);
                if (nc) put(r.cigar.data(), (size_t)nc * 4);
            }
        }
    }
    HitsBlockHead hd;
    memset(&hd, 0, sizeof(hd));
    memcpy(hd.magic, HITS_MAGIC, 4);
    hd.version = HITS_VERSION;
    hd.k = h->k; hd.want_text = h->want_text; hd.n_reads = hi - lo; hd.n_seq = (int32_t)h->lens.size(); hd.n_parts = h->n_parts;
    hd.payload = payload;
    hd.check = hits_check(base + sizeof(HitsBlockHead), payload);
    memcpy(base, &hd, sizeof(hd));
    return need;
}

// Every check runs before the accumulator is touched: a refused block leaves it as it was.
extern "C" int mpn_hits_import(mpn_hits *h, const void *buf, int64_t len, int32_t n_parts, int32_t n_seq, const char *const *names,
                               const int32_t *lens) {
    if (!h || (!buf && len > 0) || len < 0) { set_error("mpn_hits_import: null accumulator or buffer"); return -1; }
    if (n_parts < 0 || n_seq < 0 || (n_seq > 0 && (!names || !lens))) { set_error("mpn_hits_import: bad target list (n_parts %d, n_seq %d)", n_parts, n_seq); return -1; }
    HitsBlockHead hd;
    if (len < (int64_t)sizeof(hd)) { set_error("mpn_hits_import: block of %lld bytes is shorter than its header", (long long)len); return -1; }
    memcpy(&hd, buf, sizeof(hd));
    if (memcmp(hd.magic, HITS_MAGIC, 4) != 0 || hd.version != HITS_VERSION) { set_error("mpn_hits_import: not a hits block (bad magic or version)"); return -1; }
    if (hd.payload != len - (int64_t)sizeof(hd)) { set_error("mpn_hits_import: block says %lld payload bytes, %lld given", (long long)hd.payload, (long long)(len - (int64_t)sizeof(hd))); return -1; }
    const uint8_t *const p0 = (const uint8_t *)buf + sizeof(hd);
    if (hits_check(p0, hd.payload) != hd.check) { set_error("mpn_hits_import: corrupted block (checksum)"); return -1; }
    if (hd.want_text != h->want_text) { set_error("mpn_hits_import: block %s CIGARs, the accumulator %s them", hd.want_text ? "carries" : "lacks", h->want_text ? "wants" : "does not want"); return -1; }
    if (h->n_parts > 0 && hd.k != h->k) { set_error("mpn_hits_import: block of k = %d into an accumulator of k = %d", hd.k, h->k); return -1; }
    if (hd.n_reads != h->n_reads) { set_error("mpn_hits_import: block of %d reads into an accumulator of %d", hd.n_reads, h->n_reads); return -1; }
    if (hd.n_seq != n_seq || hd.n_parts != n_parts) { set_error("mpn_hits_import: block of %d targets in %d parts, %d in %d given", hd.n_seq, hd.n_parts, n_seq, n_parts); return -1; }
    for (int32_t i = 0; i < n_seq; ++i)
        if (!names[i] || lens[i] < 0) { set_error("mpn_hits_import: target %d has no name or a negative length", i); return -1; }
    // pass 1: walk the payload with every length checked against what is left, and the fields the text writers index with
    const uint8_t *p = p0, *const end = p0 + hd.payload;
    int32_t f[HIT_FIELDS];
    auto take = [&](void *dst, int64_t bytes) { if (bytes < 0 || end - p < bytes) return false; memcpy(dst, p, (size_t)bytes); p += bytes; return true; };
    for (int32_t i = 0; i < hd.n_reads; ++i) {
        int32_t rh[2];
        if (!take(rh, 8) || rh[1] < 0) { set_error("mpn_hits_import: truncated block (read %d)", i); return -1; }
        for (int32_t j = 0; j < rh[1]; ++j) {
            if (!take(f, sizeof(f))) { set_error("mpn_hits_import: truncated block (read %d, hit %d)", i, j); return -1; }
            if (f[1] < 0 || f[1] >= n_seq || (uint32_t)f[10] > 1 || f[4] < 0 || f[5] < f[4] || f[6] < 0 || f[7] < f[6]) {
                set_error("mpn_hits_import: corrupted hit (read %d, hit %d)", i, j); return -1;
            }
            if (hd.want_text) {
                int32_t nc;
                if (!take(&nc, 4) || nc < 0 || end - p < 4 * (int64_t)nc) { set_error("mpn_hits_import: truncated CIGAR (read %d, hit %d)", i, j); return -1; }
                for (int32_t c = 0; c < nc; ++c) {
                    uint32_t op;
                    memcpy(&op, p + 4 * (size_t)c, 4);
                    if ((op & 0xf) > 5) { set_error("mpn_hits_import: corrupted CIGAR (read %d, hit %d)", i, j); return -1; }
                }
                p += 4 * (size_t)nc;
            }
        }
    }
    if (p != end) { set_error("mpn_hits_import: %lld bytes past the last read", (long long)(end - p)); return -1; }
    // pass 2: append, as mpn_map_batch_parts appends the hits of the exporter's parts
    const int32_t rid0 = (int32_t)h->lens.size();
    p = p0;
    for (int32_t i = 0; i < hd.n_reads; ++i) {
        int32_t rh[2];
        take(rh, 8);
        std::vector<Reg> &regs = h->regs[(size_t)i];
        regs.reserve(regs.size() + (size_t)rh[1]);
        for (int32_t j = 0; j < rh[1]; ++j) {
            take(f, sizeof(f));
            regs.emplace_back();
            Reg &r = regs.back();
            hit_from_fields(f, r);
            r.rid += rid0;
            if (hd.want_text) {
                int32_t nc = 0;
                take(&nc, 4);
                r.cigar.resize((size_t)nc);
                if (nc) take(r.cigar.data(), 4 * (int64_t)nc);
            }
        }
        h->rep_len[(size_t)i] = std::max(h->rep_len[(size_t)i], rh[0]);
    }
    for (int32_t i = 0; i < n_seq; ++i) { h->names.emplace_back(names[i]); h->lens.push_back(lens[i]); }
    h->k = hd.k;
    h->n_parts += n_parts;
    return 0;
}
