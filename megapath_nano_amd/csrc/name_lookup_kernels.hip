// Read names matched on the resident FASTQ text, behind include/mpn_ingest.h (mpn_name_set_create, mpn_name_set_free,
// mpn_fastq_name_lookup): what `nanosplit` and `seqtk subseq` (fastx.py) need to know of a scanned text -- which entry of a name
// list each record is -- without the ids leaving the device.
//   mpn_name_set_create    builds the table and the pool of name_set_core.h on the host (serial, no atomics) and uploads them.
//   name_lookup_kernel     a lane per record: the id where it lies in the text, as 16-byte words by load16_at / load16_head of
//                          gather16.h at any alignment; ns_hash, then ns_find along the probe chain.  A slot is one 16-byte load; the
//                          pooled name is loaded (aligned words) only behind a slot whose hash and length are the id's.
// Every vector that is loaded from the text holds at least one byte of an id the host has checked against text_len.
#include "name_set_dev.h"

namespace mpn {

thread_local double tl_lookup_ms = 0;    // device time of the last mpn_fastq_name_lookup on this thread

// text_al: the text's pointer rounded down to 16 bytes, shift: what was taken off it
__global__ __launch_bounds__(256) void name_lookup_kernel(const uint4 *__restrict__ text_al, int64_t shift, const mpn_fastq_head *__restrict__ heads,
                                                          int64_t n, const NsSlot *__restrict__ table, uint32_t mask,
                                                          const uint4 *__restrict__ pool, int32_t *__restrict__ found) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const mpn_fastq_head h = heads[r];
    const NsTextWords id{text_al, h.off + shift, h.id_len};
    found[r] = ns_find(table, mask, ns_hash(h.id_len, id), h.id_len, id, NsDevPool{pool});
}

}  // namespace mpn

using namespace mpn;

extern "C" void mpn_fastq_lookup_last_device_ms(double *lookup_ms) {
    if (lookup_ms) *lookup_ms = tl_lookup_ms;
}

extern "C" void mpn_name_set_free(mpn_name_set *set) {
    if (!set) return;
    if (set->d_table) (void)hipFree(set->d_table);
    if (set->d_pool) (void)hipFree(set->d_pool);
    delete set;
}

extern "C" int32_t mpn_name_set_create(int64_t n, const char *pool, const int64_t *off, int64_t slots, mpn_name_set **set, int32_t *first_of) {
    if (!set) { set_error("mpn_name_set_create: bad arguments"); return -2; }
    *set = nullptr;
    NsBuilt built;
    try {
        const char *what = "";
        if (ns_build(n, pool, off, slots, built, first_of, &what)) { set_error("mpn_name_set_create: %s", what); return -2; }
    } catch (const std::bad_alloc &) {
        set_error("mpn_name_set_create: out of host memory");
        return -1;
    }
    mpn_name_set *s = new mpn_name_set;
    s->slots = (int64_t)built.table.size();
    s->n = n;
    s->distinct = built.distinct;
    const size_t table_bytes = built.table.size() * sizeof(NsSlot), pool_bytes = std::max<size_t>(built.pool.size(), 1) * sizeof(NsWord);
    hipError_t e = hipMalloc((void **)&s->d_table, table_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_pool, pool_bytes);
    if (e == hipSuccess) e = hipMemcpy(s->d_table, built.table.data(), table_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && !built.pool.empty()) e = hipMemcpy(s->d_pool, built.pool.data(), built.pool.size() * sizeof(NsWord), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        set_error("mpn_name_set_create: %s", hipGetErrorString(e));
        (void)hipGetLastError();
        mpn_name_set_free(s);
        return -1;
    }
    *set = s;
    return 0;
}

extern "C" int32_t mpn_fastq_name_lookup(const void *d_text, int64_t text_len, int64_t n, const mpn_fastq_head *heads, const mpn_name_set *set,
                                         int32_t *found) {
    tl_lookup_ms = 0;
    if (n < 0 || n > 0x7fffffff || text_len < 0 || !set || (n > 0 && (!heads || !found || !d_text))) {
        set_error("mpn_fastq_name_lookup: bad arguments");
        return -2;
    }
    for (int64_t r = 0; r < n; ++r) {
        const mpn_fastq_head &h = heads[r];
        if (h.off < 0 || h.id_len < 0 || h.off > text_len - h.id_len) {
            set_error("mpn_fastq_name_lookup: the id of record %lld does not lie in the text", (long long)r);
            return -2;
        }
    }
    if (n == 0) return 0;
    hipStream_t st = 0;
    DevBuf<mpn_fastq_head> d_heads;
    DevBuf<int32_t> d_found;
    DevTimer tm;
    if (d_heads.upload(heads, (size_t)n, st) || d_found.alloc((size_t)n) || tm.start(st)) return -1;
    const uintptr_t shift = (uintptr_t)d_text & 15;
    hipLaunchKernelGGL(name_lookup_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const uint4 *)((const uint8_t *)d_text - shift),
                       (int64_t)shift, (const mpn_fastq_head *)d_heads.p, n, (const NsSlot *)set->d_table, (uint32_t)(set->slots - 1),
                       (const uint4 *)set->d_pool, d_found.p);
    MPN_HIP_CHECK(hipGetLastError());
    if (tm.stop(st) || d_found.download(found, (size_t)n, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    return tm.elapsed_ms(&tl_lookup_ms);
}
