/*
 * mpn_dbg.h -- C-ABI of the MI355X-native de Bruijn graph consensus (libmpn.so): the candidate haplotypes of a window, which the
 * amplicon realigner (mpn_realign.h) takes as its input.
 *
 * It restates the reference's realign/debruijn_graph.cpp (DeBruijnGraph::Build and what it calls) without Boost: for k = 10 .. min(101,
 * reference length - 1), the first k at which the reference's k-mers are distinct and the graph of reference and reads has no cycle is
 * pruned (reference edges and edges that two reads walk; vertices between source and sink) and walked breadth-first from the
 * reference's first k-mer, with the reference's cap of 256 live paths; the haplotypes are returned sorted bytewise.  The rules are in
 * csrc/dbg_core.h, one text for the kernel (csrc/dbg_kernels.hip; one workgroup owns a window and runs its whole k loop) and for the
 * host check (scripts/dbg_host_check.cpp).  There is no CPU fallback.
 *
 * One point of the reference is not reproducible in the reference itself: its adjacency order is pointer order, and the outcome
 * depends on it when the path count passes 256 through the successors of the very last path popped.  This port walks successors in
 * ascending k-mer order.
 *
 * Limits, refused before anything is uploaded (negative return or NULL, text in mpn_last_error()):
 *   a reference longer than MPN_DBG_MAX_REF bases (the reference's script never builds a window over 1000);
 *   a window whose reference and reads together pass MPN_DBG_MAX_WINDOW_BASES;
 *   a call whose smallest workspace (one workgroup's tables for its largest window) passes MPN_DBG_WORKSPACE_BUDGET bytes.
 */
#ifndef MPN_DBG_H
#define MPN_DBG_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPN_DBG_MAX_REF 1000
#define MPN_DBG_MAX_WINDOW_BASES (1 << 24)
#define MPN_DBG_WORKSPACE_BUDGET ((int64_t)8 << 30)

/* ---- Part 1: reference-compatible entry ----------------------------------------------- */
typedef struct {              /* debruijn_graph.h: struct_str_arr there; that name is the realigner's in this library */
    int consensus_size;
    char *consensus[500];
} mpn_dbg_str_arr;

/* reference: the window; c_reads: the reads joined with ','; c_base_quality: per read, joined with ',', its low-quality positions
 * as integers separated by white space (more lists than reads are ignored, fewer are refused); read_size is not read, as in the
 * reference.  Returns a new mpn_dbg_str_arr with consensus_size strings, or NULL; release it with free_consensus(ptr, size)
 * (the reference's free_memory: that name, too, is the realigner's here). */
mpn_dbg_str_arr *get_consensus(char *reference, char *c_reads, char *c_base_quality, int read_size);
void free_consensus(mpn_dbg_str_arr *pointer, int size);

/* ---- Part 2: batched form --------------------------------------------------------------- */
typedef struct {
    const char *reference;         /* NUL-terminated; any bytes, compared as bytes */
    int32_t n_reads;
    const char *const *reads;      /* n_reads NUL-terminated reads (may be empty strings) */
    const uint8_t *const *bad;     /* NULL, or n_reads entries: NULL, or one byte per base of the read, nonzero = low quality */
} mpn_dbg_window;

enum {
    MPN_DBG_OK = 0,          /* k found: n_haps haplotypes of its graph (possibly none) */
    MPN_DBG_NO_K = 1,        /* no usable k: no haplotypes, k = 0 */
    MPN_DBG_PATH_CAP = 2,    /* k found, over 256 live paths: no haplotypes */
    MPN_DBG_TABLE_FULL = 3,  /* the window's tables would pass the workspace budget: refused, nothing cut short */
    MPN_DBG_HAP_FULL = 4     /* likewise, for its haplotype buffers */
};

typedef struct {
    int32_t status, k, n_haps;
    char **haps;                   /* n_haps NUL-terminated strings, sorted; NULL when there are none */
} mpn_dbg_result;

/* One result per window.  table_cap: the largest k-mer table (slots) a window starts with, grid_cap: the largest grid; 0 for the
 * library's own values (both are test knobs: a table that turns out too small is enlarged and the window done again, which
 * *out_redone counts, if not NULL).  Results do not depend on either knob, on the other windows of the call or on the run.
 * Returns 0, or a negative code with mpn_last_error() and nothing written; release the strings with mpn_dbg_free_results. */
int mpn_dbg_consensus_batch(int32_t n_windows, const mpn_dbg_window *windows, int64_t table_cap, int32_t grid_cap,
                            mpn_dbg_result *out, int32_t *out_redone);
void mpn_dbg_free_results(mpn_dbg_result *results, int32_t n);

/* device time of the calling thread's last mpn_dbg_consensus_batch: all passes of the kernel, in milliseconds */
void mpn_dbg_last_device_ms(double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif
