// Host build of the mapper's host hit path and of the hits block format: csrc/hit_host.cpp and csrc/hits_block.cpp linked into a
// program of its own for tests/test_hit_host.py (under AddressSanitizer and UBSan).
//
//   hit_host_check hits  <cases> <results>   every read through gen_regs, set_parent, select_sub, squeeze_a, join_long, in the order
//                                            and with the glue of hits_from_chains' host path (csrc/align.hip)
//   hit_host_check block <cases> <results>   an accumulator of given hits exported, imported twice into a fresh one, and every
//                                            truncation and single-byte change of the block offered to mpn_hits_import
//
// hits <cases>, little endian: u32 n_batches, then per batch u32 opt_size, the bytes of its mpn_map_opt, i32 k, u32 n_reads, per read
//   i32 name_len (-1: no name), name, i32 qlen, u32 n_chains, per chain in pool order u64 u, fx, fy, lx, ly, i32 mlen, blen
// hits <results>: per read i32 n_regs, n_a, n_segs; per hit 15 i64 (the words of mpn_hit_select_batch: fx, fy, lx, ly, score, score0,
//   cnt, as, parent, subsc, n_sub, mlen, blen, hash, sam_pri); per segment i64 src (from the read's first pool anchor), i32 dst, cnt, flag
// block <cases>: i32 k, want_text, n_parts, n_seq, per target i32 len (its name is "t<i>"), i32 n_reads, per read i32 rep_len, n_hits,
//   per hit 18 i32 (the block's fields), i32 n_cigar, the CIGAR words; i32 lo, hi
// block <results>: i64 block bytes, then the fresh accumulator after the two imports: i32 k, n_parts, n_seq, the lens, per read i32
//   rep_len, n_hits, per hit the 18 fields, i32 n_cigar, the words; then i64 truncations refused, payload changes refused, check-field
//   changes refused, other header changes accepted, other header changes refused.  Any failed expectation ends the run with status 1.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../megapath_nano_amd/csrc/hit_host.h"

namespace mpn {
static char g_err[512];
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace mpn
using namespace mpn;

struct In {
    std::vector<uint8_t> b;
    size_t p = 0;
    bool ok = true;
    void take(void *dst, size_t n) { if (n == 0) return; if (!ok || b.size() - p < n) { ok = false; memset(dst, 0, n); return; } memcpy(dst, b.data() + p, n); p += n; }
    template <typename T> T get() { T v; take(&v, sizeof(T)); return v; }
};
static bool slurp(const char *path, In &in) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) in.b.insert(in.b.end(), buf, buf + n);
    fclose(f);
    return true;
}
struct Out {
    std::string s;
    void put(const void *p, size_t n) { if (n) s.append((const char *)p, n); }
    template <typename T> void val(T v) { put(&v, sizeof(T)); }
    bool save(const char *path) const {
        FILE *f = fopen(path, "wb");
        if (!f) return false;
        const bool ok = fwrite(s.data(), 1, s.size(), f) == s.size();
        return fclose(f) == 0 && ok;
    }
};
static int fail(const char *what) { fprintf(stderr, "hit_host_check: %s (%s)\n", what, g_err); return 1; }

// ---- the host hit path ------------------------------------------------------------------------------------------------------
static int run_hits(In &in, Out &out) {
    const uint32_t n_batches = in.get<uint32_t>();
    std::vector<ChainRec> recs;
    std::vector<uint64_t> u;
    std::vector<ChainIn> cin;
    std::vector<std::pair<std::pair<uint64_t, uint64_t>, int>> w;
    for (uint32_t b = 0; in.ok && b < n_batches; ++b) {
        mpn_map_opt opt;
        if (in.get<uint32_t>() != sizeof(opt)) return fail("the options are not this build's mpn_map_opt");
        in.take(&opt, sizeof(opt));
        const int32_t k = in.get<int32_t>();
        const uint32_t n_reads = in.get<uint32_t>();
        for (uint32_t i = 0; in.ok && i < n_reads; ++i) {
            const int32_t name_len = in.get<int32_t>();
            std::string name((size_t)std::max(0, name_len), '\0');
            in.take(&name[0], name.size());
            const int32_t qlen = in.get<int32_t>();
            const uint32_t nc = in.get<uint32_t>();
            if (!in.ok || nc > in.b.size()) return fail("truncated case file");
            recs.resize(nc); u.resize(nc);
            for (uint32_t c = 0; c < nc; ++c) {
                u[c] = in.get<uint64_t>();
                ChainRec &r = recs[c];
                r.fx = in.get<uint64_t>(); r.fy = in.get<uint64_t>(); r.lx = in.get<uint64_t>(); r.ly = in.get<uint64_t>();
                r.mlen = in.get<int32_t>(); r.blen = in.get<int32_t>();
            }
            if (!in.ok) return fail("truncated case file");
            ReadState S;
            std::vector<SqueezeSeg> segs;
            if (nc > 0) {
                // HostChains::chain_order: the chains by first anchor, then place in the pool; src = where the chain's anchors start
                w.resize(nc);
                int64_t at = 0;
                for (uint32_t c = 0; c < nc; ++c) { w[c] = {{recs[c].fx, (uint64_t)at << 32 | c}, (int)c}; at += (int32_t)u[c]; }
                std::sort(w.begin(), w.end());
                cin.resize(nc);
                for (uint32_t c = 0; c < nc; ++c) cin[c] = ChainIn{u[(size_t)w[c].second], &recs[(size_t)w[c].second], (int64_t)(w[c].first.second >> 32)};
                // the host path of hits_from_chains
                uint32_t hash = name_len >= 0 ? x31_hash(name.c_str()) : 0;
                hash ^= wang32((uint32_t)qlen) + wang32(opt.seed);
                hash = wang32(hash);
                gen_regs(hash, qlen, (int)nc, cin.data(), S.regs);
                set_parent(opt.mask_level, S.regs, opt.a * 2 + opt.b);
                select_sub(opt.pri_ratio, k * 2, opt.best_n, S.regs);
                S.n_a = squeeze_a(S.regs, (int)i, 0, segs);
                join_long(&opt, qlen, S.regs, segs);
                if (!opt.with_cigar) segs.clear();
            }
            out.val<int32_t>((int32_t)S.regs.size()); out.val<int32_t>(S.n_a); out.val<int32_t>((int32_t)segs.size());
            for (const Reg &r : S.regs) {
                const int64_t o[15] = {(int64_t)r.fx, (int64_t)r.fy, (int64_t)r.lx, (int64_t)r.ly, r.score, r.score0, r.cnt, r.as, r.parent, r.subsc, r.n_sub,
                                       r.mlen, r.blen, (int64_t)r.hash, (int64_t)r.sam_pri};
                out.put(o, sizeof(o));
            }
            for (const SqueezeSeg &s : segs) { out.val<int64_t>(s.src); out.val<int32_t>(s.dst); out.val<int32_t>(s.cnt); out.val<int32_t>(s.flag); }
        }
    }
    return in.ok && in.p == in.b.size() ? 0 : fail("truncated case file, or bytes behind its end");
}

// ---- the hits block ---------------------------------------------------------------------------------------------------------
static const int N_FIELDS = 18;
static void fields_of(const Reg &r, int32_t *f) {
    const int32_t v[N_FIELDS] = {r.cnt, r.rid, r.score, r.score0, r.qs, r.qe, r.rs, r.re, r.mlen, r.blen, (int32_t)r.rev, (int32_t)r.inv,
                                 (int32_t)r.split, (int32_t)r.hash, r.has_p, r.dp_score, r.dp_max, r.n_ambi};
    memcpy(f, v, sizeof(v));
}
// everything an import may change, as bytes
static void dump(const mpn_hits *h, Out &o, bool with_names) {
    o.val<int32_t>(h->k); o.val<int32_t>(h->n_parts); o.val<int32_t>((int32_t)h->lens.size());
    for (int32_t l : h->lens) o.val<int32_t>(l);
    if (with_names) for (const std::string &s : h->names) { o.val<int32_t>((int32_t)s.size()); o.put(s.data(), s.size()); }
    for (int32_t i = 0; i < h->n_reads; ++i) {
        o.val<int32_t>(h->rep_len[(size_t)i]); o.val<int32_t>((int32_t)h->regs[(size_t)i].size());
        for (const Reg &r : h->regs[(size_t)i]) {
            int32_t f[N_FIELDS];
            fields_of(r, f);
            o.put(f, sizeof(f));
            o.val<int32_t>((int32_t)r.cigar.size());
            o.put(r.cigar.data(), r.cigar.size() * 4);
        }
    }
}
struct Acc {
    mpn_hits *h;
    explicit Acc(int32_t n) : h(mpn_hits_create(n)) {}
    Acc(const Acc &) = delete;
    Acc &operator=(const Acc &) = delete;
    ~Acc() { mpn_hits_destroy(h); }
};

static int run_block(In &in, Out &out) {
    const int32_t k = in.get<int32_t>(), want_text = in.get<int32_t>(), n_parts = in.get<int32_t>(), n_seq = in.get<int32_t>();
    if (!in.ok || n_seq < 0 || (size_t)n_seq > in.b.size()) return fail("truncated case file");
    std::vector<int32_t> lens((size_t)n_seq);
    std::vector<std::string> names;
    for (int32_t t = 0; t < n_seq; ++t) { lens[(size_t)t] = in.get<int32_t>(); names.push_back("t" + std::to_string(t)); }
    std::vector<const char *> name_p;
    for (const std::string &s : names) name_p.push_back(s.c_str());
    const int32_t n_reads = in.get<int32_t>();
    if (!in.ok || n_reads < 0 || (size_t)n_reads > in.b.size()) return fail("truncated case file");
    Acc src(n_reads);
    if (!src.h) return fail("mpn_hits_create");
    mpn_hits_set_text(src.h, want_text);
    src.h->k = k; src.h->n_parts = n_parts; src.h->names = names; src.h->lens = lens;
    for (int32_t i = 0; i < n_reads; ++i) {
        src.h->rep_len[(size_t)i] = in.get<int32_t>();
        const int32_t n_hits = in.get<int32_t>();
        if (!in.ok || n_hits < 0 || (size_t)n_hits > in.b.size()) return fail("truncated case file");
        for (int32_t j = 0; j < n_hits; ++j) {
            int32_t f[N_FIELDS];
            in.take(f, sizeof(f));
            Reg r;
            r.cnt = f[0]; r.rid = f[1]; r.score = f[2]; r.score0 = f[3]; r.qs = f[4]; r.qe = f[5]; r.rs = f[6]; r.re = f[7]; r.mlen = f[8]; r.blen = f[9];
            r.rev = (uint32_t)f[10]; r.inv = (uint32_t)f[11]; r.split = (uint32_t)f[12]; r.hash = (uint32_t)f[13]; r.has_p = f[14]; r.dp_score = f[15];
            r.dp_max = f[16]; r.n_ambi = f[17];
            const int32_t nc = in.get<int32_t>();
            if (!in.ok || nc < 0 || (size_t)nc > in.b.size()) return fail("truncated case file");
            r.cigar.resize((size_t)nc);
            in.take(r.cigar.data(), (size_t)nc * 4);
            src.h->regs[(size_t)i].push_back(r);
        }
    }
    const int32_t lo = in.get<int32_t>(), hi = in.get<int32_t>();
    if (!in.ok || in.p != in.b.size()) return fail("truncated case file, or bytes behind its end");

    const int64_t need = mpn_hits_export(src.h, lo, hi, nullptr, 0);
    if (need <= 0) return fail("mpn_hits_export: size query");
    std::vector<uint8_t> block((size_t)need);
    if (mpn_hits_export(src.h, lo, hi, block.data(), need - 1) != -3) return fail("mpn_hits_export took a buffer one byte short");
    if (mpn_hits_export(src.h, lo, hi, block.data(), need) != need) return fail("mpn_hits_export");
    out.val<int64_t>(need);

    // two imports into a fresh accumulator: the second finds the targets of the first and shifts its target ids behind them
    Acc dst(hi - lo);
    mpn_hits_set_text(dst.h, want_text);
    for (int pass = 0; pass < 2; ++pass)
        if (mpn_hits_import(dst.h, block.data(), need, n_parts, n_seq, name_p.data(), lens.data())) return fail("mpn_hits_import of the exported block");
    if (dst.h->names.size() != 2 * names.size() || !std::equal(names.begin(), names.end(), dst.h->names.begin()) ||
        !std::equal(names.begin(), names.end(), dst.h->names.begin() + n_seq))
        return fail("the imported target names");
    dump(dst.h, out, false);

    // every refusal leaves the accumulator as it was
    Out before;
    dump(dst.h, before, true);
    auto refused_unchanged = [&](const std::vector<uint8_t> &blk, int64_t len) {
        if (mpn_hits_import(dst.h, blk.data(), len, n_parts, n_seq, name_p.data(), lens.data()) != -1) return false;
        Out after;
        dump(dst.h, after, true);
        return after.s == before.s;
    };
    int64_t n_trunc = 0, n_payload = 0, n_check = 0, n_head_ok = 0, n_head_no = 0;
    for (int64_t len = 0; len < need; ++len) {   // (a copy of exactly len bytes: a read behind it is a read behind the allocation)
        const std::vector<uint8_t> cut(block.begin(), block.begin() + len);
        if (!refused_unchanged(cut, len)) return fail("a truncated block was accepted, or changed the accumulator");
        ++n_trunc;
    }
    const int64_t head = 48, check_at = 40;   // HitsBlockHead: the check field is its last word, the payload follows
    std::vector<uint8_t> bad = block;
    for (int64_t at = 0; at < need; ++at) {
        for (int v = 1; v < 256; ++v) {
            bad[(size_t)at] = (uint8_t)(block[(size_t)at] ^ v);
            if (at >= check_at) {
                if (!refused_unchanged(bad, need)) return fail("a block with a changed payload or check byte was accepted, or changed the accumulator");
                ++(at >= head ? n_payload : n_check);
            } else {
                // other header bytes: the block may still be a valid one (the pad word); what matters is a clean run, and that a
                // refusal changes nothing
                Acc tmp(hi - lo);
                mpn_hits_set_text(tmp.h, want_text);
                Out b0, b1;
                dump(tmp.h, b0, true);
                const int rc = mpn_hits_import(tmp.h, bad.data(), need, n_parts, n_seq, name_p.data(), lens.data());
                dump(tmp.h, b1, true);
                if (rc != 0 && b0.s != b1.s) return fail("a refused block changed the accumulator");
                ++(rc == 0 ? n_head_ok : n_head_no);
            }
        }
        bad[(size_t)at] = block[(size_t)at];
    }
    out.val<int64_t>(n_trunc); out.val<int64_t>(n_payload); out.val<int64_t>(n_check); out.val<int64_t>(n_head_ok); out.val<int64_t>(n_head_no);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 4 || (strcmp(argv[1], "hits") && strcmp(argv[1], "block"))) { fprintf(stderr, "usage: hit_host_check hits|block <cases> <results>\n"); return 2; }
    In in;
    if (!slurp(argv[2], in)) { fprintf(stderr, "hit_host_check: cannot read %s\n", argv[2]); return 2; }
    Out out;
    const int rc = strcmp(argv[1], "hits") == 0 ? run_hits(in, out) : run_block(in, out);
    if (rc) return rc;
    return out.save(argv[3]) ? 0 : 2;
}
