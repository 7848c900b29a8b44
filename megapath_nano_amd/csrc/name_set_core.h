// The name set of mpn_name_set_create / mpn_fastq_name_lookup (include/mpn_ingest.h): hash, probe step, slot layout and the host
// builder.  Like inflate_core.h and bam_walk_core.h it compiles for the device (a lane of csrc/name_lookup_kernels.hip probes with
// ns_hash and ns_find) and for the host with plain g++ (scripts/name_set_host_check.cpp builds sets and probes them with the same
// functions; mpn_name_set_create builds with ns_build).
//
// Bytes as words.  A name of len bytes is read as (len + 15) / 16 WORDS of 16 bytes, the last one filled up with zero bytes; a word
// is four little-endian uint32 (NsWord).  The device gets the words of an id in the text by the 16-byte loads of gather16.h at any
// alignment, the pooled names are stored as such words, and the host makes them with memcpy (little-endian hosts only).
//
// Hash (32 bits): h = NS_SEED; per word, per uint32 v of it in order: h = rotl(h ^ v, 13) * 0x9E3779B1 (wrapping); at the end
// h ^= len, then the finaliser of MurmurHash3 (h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16).  The
// length goes in because of the zero fill: "a" and "a\0" have equal words.  The empty name hashes to the finaliser of NS_SEED.
//
// Table: `slots` (a power of two) entries of 16 bytes, open addressing.  A name's home is hash & (slots - 1); the probe step is +1,
// wrapping at the end of the table; a probe ends at the name or at the first empty slot (at least one slot is always empty).
//   NsSlot.index   the SMALLEST list index with these bytes; -1: the slot is empty
//   NsSlot.hash    all 32 bits of the hash: a slot whose hash or length differs costs no load from the pool
//   NsSlot.off16   where the name's words start in the pool, in words
//   NsSlot.len     its bytes
// Pool: the words of the distinct names one behind the other, in the order of their smallest index (an empty name has none).
// The builder is serial host code without atomics: names enter in list order, so the layout depends on the list and on `slots` alone.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define NS_HD __host__ __device__ __forceinline__
#else
#define NS_HD inline
#endif

namespace mpn {

struct NsWord { uint32_t x, y, z, w; };
struct alignas(16) NsSlot { int32_t index; uint32_t hash; uint32_t off16; int32_t len; };
static_assert(sizeof(NsSlot) == 16 && sizeof(NsWord) == 16, "a slot and a word are one 16-byte load each");

constexpr uint32_t NS_SEED = 0x9E3779B9u;
constexpr int64_t NS_MIN_SLOTS = 16, NS_MAX_SLOTS = (int64_t)1 << 31;

NS_HD uint32_t ns_words(int32_t len) { return ((uint32_t)len + 15u) >> 4; }
NS_HD uint32_t ns_mix(uint32_t h, uint32_t v) {
    h ^= v;
    h = (h << 13) | (h >> 19);
    return h * 0x9E3779B1u;
}
NS_HD bool ns_same(const NsWord &a, const NsWord &b) { return ((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) == 0; }

// Words: anything with  NsWord operator()(uint32_t k) const  -- word k of the name
template <class Words>
NS_HD uint32_t ns_hash(int32_t len, const Words &name) {
    uint32_t h = NS_SEED;
    for (uint32_t k = 0, nw = ns_words(len); k < nw; ++k) {
        const NsWord w = name(k);
        h = ns_mix(ns_mix(ns_mix(ns_mix(h, w.x), w.y), w.z), w.w);
    }
    h ^= (uint32_t)len;
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

// The probe.  id: the words of the bytes that are looked up; pool: word k of the POOL (k counts from the pool's start).
// -> the index in the slot that holds the name, or -1; *at: that slot, or the empty slot that ends the chain (the builder puts a
// new name there).  *probes receives the slots that were read.  One round of the table at the most, even if it were full (a full
// table is never built).
template <class IdWords, class PoolWords>
NS_HD int32_t ns_probe(const NsSlot *table, uint32_t mask, uint32_t hash, int32_t len, const IdWords &id, const PoolWords &pool, uint32_t *at,
                       int64_t *probes) {
    const uint32_t nw = ns_words(len);
    uint32_t s = hash & mask;
    int32_t found = -1;
    int64_t seen = 0;
    for (uint32_t left = mask;; --left, s = (s + 1) & mask) {
        const NsSlot e = table[s];
        ++seen;
        if (e.index < 0) break;
        if (e.hash == hash && e.len == len) {
            uint32_t k = 0;
            while (k < nw && ns_same(id(k), pool(e.off16 + k))) ++k;
            if (k == nw) { found = e.index; break; }
        }
        if (left == 0) break;
    }
    *at = s;
    *probes = seen;
    return found;
}

// -> the smallest list index whose bytes are the id's, or -1
template <class IdWords, class PoolWords>
NS_HD int32_t ns_find(const NsSlot *table, uint32_t mask, uint32_t hash, int32_t len, const IdWords &id, const PoolWords &pool) {
    uint32_t at;
    int64_t probes;
    return ns_probe(table, mask, hash, len, id, pool, &at, &probes);
}

}  // namespace mpn

// ---- host code: words of host bytes, and the builder -------------------------------------------------------------------------------
#include <vector>

namespace mpn {

struct NsHostBytes {      // the words of p[0 .. len)
    const uint8_t *p;
    int32_t len;
    NsWord operator()(uint32_t k) const {
        uint32_t v[4] = {0, 0, 0, 0};
        const uint32_t at = 16 * k, left = (uint32_t)len - at;
        if (left) memcpy(v, p + at, left < 16 ? left : 16);
        return NsWord{v[0], v[1], v[2], v[3]};
    }
};
struct NsHostPool {
    const NsWord *pool;
    NsWord operator()(uint32_t k) const { return pool[k]; }
};

struct NsBuilt {
    std::vector<NsSlot> table;
    std::vector<NsWord> pool;
    int64_t distinct = 0;
};

inline int64_t ns_default_slots(int64_t distinct) {
    int64_t s = NS_MIN_SLOTS;
    while (s < 2 * distinct) s <<= 1;
    return s;
}

// Name i is pool[off[i] .. off[i + 1]).  slots: 0 = ns_default_slots(distinct), else a power of two > distinct.  first_of (n entries
// or NULL): the smallest index with the bytes of name i.  -> 0, or -2 for arguments the contract excludes (what: which).
inline int ns_build(int64_t n, const char *names, const int64_t *off, int64_t slots, NsBuilt &out, int32_t *first_of, const char **what) {
    static const char *dummy;
    if (!what) what = &dummy;
    if (n < 0 || n > 0x7fffffff || (n > 0 && !off)) { *what = "n is negative or larger than 2^31 - 1, or off is NULL"; return -2; }
    for (int64_t i = 0; i < n; ++i)
        if (off[i] < 0 || off[i + 1] < off[i] || off[i + 1] - off[i] > 0x7fffffff || (off[i + 1] > off[i] && !names)) {
            *what = "off does not ascend, a name is longer than 2^31 - 1 bytes, or pool is NULL";
            return -2;
        }
    if (slots < 0 || slots > NS_MAX_SLOTS || (slots & (slots - 1))) { *what = "slots is no power of two up to 2^31"; return -2; }
    // first pass: a table no name list can fill, which finds the equal names; the distinct ones stay in list order
    std::vector<NsSlot> wide((size_t)ns_default_slots(n), NsSlot{-1, 0, 0, 0});
    const uint32_t wmask = (uint32_t)(wide.size() - 1);
    std::vector<NsSlot> firsts;
    out.pool.clear();
    for (int64_t i = 0; i < n; ++i) {
        const int32_t len = (int32_t)(off[i + 1] - off[i]);
        const NsHostBytes id{(const uint8_t *)names + off[i], len};
        const uint32_t h = ns_hash(len, id);
        uint32_t at;
        int64_t probes;
        ns_probe(wide.data(), wmask, h, len, id, NsHostPool{out.pool.data()}, &at, &probes);
        NsSlot &e = wide[at];
        if (e.index < 0) {
            if (out.pool.size() + ns_words(len) > 0xffffffffu) { *what = "the names need more than 2^32 words of 16 bytes"; return -2; }
            e = NsSlot{(int32_t)i, h, (uint32_t)out.pool.size(), len};
            for (uint32_t k = 0; k < ns_words(len); ++k) out.pool.push_back(id(k));
            firsts.push_back(e);
        }
        if (first_of) first_of[i] = e.index;
    }
    out.distinct = (int64_t)firsts.size();
    if (slots == 0) slots = ns_default_slots(out.distinct);
    if (slots <= out.distinct) { *what = "slots is not larger than the number of distinct names"; return -2; }
    // second pass: the distinct names into the table that was asked for, smallest index first, each at the end of its chain
    out.table.assign((size_t)slots, NsSlot{-1, 0, 0, 0});
    const uint32_t mask = (uint32_t)(slots - 1);
    for (const NsSlot &e : firsts) {
        uint32_t s = e.hash & mask;
        while (out.table[s].index >= 0) s = (s + 1) & mask;
        out.table[s] = e;
    }
    return 0;
}

}  // namespace mpn
