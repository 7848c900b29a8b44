/* Regrouping a batch of packed reads on the device (the reference's bin/tools/nanosplit, which cuts a run's
 * FASTQ into one file per species between species placement and the per-species mapping calls of step_placement_to_assembly,
 * bin/megapath_nano.py:1313-1397).  The layout is the one mpn_map_batch_ex takes: concatenated ASCII, off, len, and optionally
 * qualities with the same offsets.
 *
 * n reads are regrouped into n_groups groups from m membership pairs (read, group), with nanosplit's semantics: a read may be
 * in several groups or in none; a pair given twice counts once; within a group the reads keep their input order (ascending read
 * index), whatever the order of the pairs.
 *
 * Output layout: every group's block starts at a multiple of 16 bytes, so that a group is a valid d_seqs of its own; the reads
 * of a group lie back to back; out_bytes = group_byte[n_groups] + 16, a multiple of 16 that leaves at least 4 readable bytes
 * after the last base of every group (the mapper reads the aligned 32-bit word around a batch's last base).
 *
 * All calls return 0, or -1 with mpn_last_error(); arguments are validated on the host before anything is launched. */
#ifndef MPN_READS_H
#define MPN_READS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPN_SPLIT_ALIGN 16   /* a group's block starts at a multiple of this */
#define MPN_SPLIT_CHUNK 1024 /* bytes of output a wave writes per step of the gather: 64 lanes x 16 B */

/* The plan, on the device: stable radix sort of (group, read) keys, adjacent-unique flags, a scan for the compaction, a
 * segmented scan of the lengths per group and a scan of the groups' sizes rounded up to MPN_SPLIT_ALIGN.
 * len[n]: read lengths (>= 0).  mem_read[m] in [0, n), mem_group[m] in [0, n_groups).  out_cap: capacity of out_read and out_off
 * (m always suffices).  Outputs (host arrays): *n_out distinct pairs; out_read[n_out] the source read of every output read,
 * group after group; group_first[n_groups + 1] a CSR over output reads; out_off[n_out] byte offsets into the output buffer;
 * group_byte[n_groups + 1] where each group's block starts (the last entry: where the last block ends, rounded up); *out_bytes
 * the size of the output buffer.  n = 0, m = 0 and empty groups are valid. */
int mpn_reads_split_plan(int32_t n, const int32_t *len, int64_t m, const int32_t *mem_read, const int32_t *mem_group, int32_t n_groups,
                         int64_t out_cap, int64_t *n_out, int32_t *out_read, int64_t *group_first, int64_t *out_off,
                         int64_t *group_byte, int64_t *out_bytes);

/* The gather.  seqs (and quals, or NULL): src_bytes bytes each; host pointers, or with src_on_device DEVICE pointers aligned to
 * 16 bytes whose allocation is readable up to src_bytes rounded up to 4.  off[n], len[n]: host arrays, off[i] + len[i] <= src_bytes.
 * out_read / out_off / out_bytes: a plan (host arrays); it is checked against len: offsets ascending, no two reads overlapping,
 * everything inside [0, out_bytes).  d_out_seqs (and d_out_quals when quals is given): DEVICE buffers of d_out_cap >= out_bytes
 * bytes, aligned to 16.  h_out_seqs / h_out_quals: host buffers of out_bytes that receive a copy, or NULL.
 * Every byte of [0, out_bytes) that belongs to no read is written as 0; no byte at or beyond out_bytes is written; no load touches
 * a source beyond src_bytes rounded up to 4. */
int mpn_reads_split_gather(int32_t n, const void *seqs, const void *quals, int64_t src_bytes, const int64_t *off, const int32_t *len,
                           int32_t src_on_device, int64_t n_out, const int32_t *out_read, const int64_t *out_off, int64_t out_bytes,
                           void *d_out_seqs, void *d_out_quals, int64_t d_out_cap, void *h_out_seqs, void *h_out_quals);

/* Device time of the last plan / gather call of this thread (HIP events around the launches, transfers excluded), ns. */
int64_t mpn_reads_split_last_ns(int32_t which /* 0 plan, 1 gather */);

#ifdef __cplusplus
}
#endif
#endif
