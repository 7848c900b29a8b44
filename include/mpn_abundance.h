/*
 * mpn_abundance.h -- C-ABI of the data-parallel steps of the output formats / abundance statistic:
 *
 *   mpn_sort_order      the coordinate sort of `samtools sort` (reference, position, strand; ties in file order) that the
 *                       reference runs on the species-placement SAM   (/root/reference/bin/lib/aligner.py:246-252)
 *   mpn_cover_by_group  `bedtools sort | bedtools merge` + the per-assembly sum of the merged lengths
 *                       (/root/reference/bin/megapath_nano.py:313-347: align_list_to_bed, bed_to_covered_bp_by_assembly_id),
 *                       i.e. the covered base pairs of every assembly; the noise-BED variant (`covered_bed.subtract(noise_bed)`,
 *                       :516-518) is two calls: |A \ N| = |A u N| - |N| per sequence (megapath_nano_amd/abundance.py)
 *
 *   mpn_depth_by_key    `bedtools genomecov -bg` over the target intervals of an alignment table, the per-assembly depth
 *                       threshold on the profile rows and `bedtools sort | merge` of the rows that pass, with their summed length
 *                       per assembly (the reference's bin/megapath_nano.py:417-482: align_list_to_depth_bed, behind the spike and
 *                       variable-region noise BEDs).  bedtools is restated here, not linked or run: see DESIGN.md section 2.
 *
 *   mpn_bed_union       `bedtools sort | bedtools merge` with the merged intervals themselves as output: how the reference combines
 *                       noise BEDs (bin/megapath_nano.py:362-382: merge_bed_with_assembly_id)
 *   mpn_cover_by_bed    the counting half of `bedtools annotate`: the positions of every query interval that a BED covers, behind
 *                       the reference's select_alignment_by_bed (bin/megapath_nano.py:666-717), which applies a noise BED to
 *                       alignments.  Restated, not run, like the depth profile.
 *
 *   mpn_best_candidates      the rows that can be a read's best alignment: the best row per (read, assembly), of those the ones with
 *   mpn_pick_weighted        their read's largest score; the abundance-weighted random draw among them (the reference's
 *   mpn_second_best_by_read  bin/megapath_nano.py:244-310: align_list_to_best_align_list); the largest score of a read off its best
 *                            row's assembly (:2553-2593: step_unique_alignment).  The random numbers are an input.
 *
 *   mpn_good_rows       the best row per (read, unit) and, of those, the rows that reach a fraction of their read's best score: the
 *                       reference's good_align_list (bin/megapath_nano.py:642-663), the first half of
 *                       align_list_to_align_stat_by_sequence_id (:591) and the best row per read of step_assembly_selection (:1459)
 *   mpn_sum_by_key      the grouped integer sums of summary_stat_1 (:485-493) per assembly or per (assembly, sequence)
 *
 * All run on the GPU (csrc/interval_kernels.hip: a stable LSD radix sort of 128-bit keys, three-phase sweeps and segmented scans over
 * the sorted list); all pointers are HOST pointers, results are exact integers -- and, in mpn_pick_weighted, float64 values that one
 * IEEE division and one multiplication define; mpn_good_rows compares through one IEEE float64 product.  Return 0, or a negative
 * error (mpn_last_error()).
 */
#ifndef MPN_ABUNDANCE_H
#define MPN_ABUNDANCE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* order[0..n): the indices of the records in ascending (hi, lo); records with equal keys keep their input order (stable). */
int mpn_sort_order(int64_t n, const uint64_t *hi, const uint64_t *lo, int64_t *order);

/* covered[g] (g < n_groups, zeroed by the call) = sum over the sequences of group g of the length of the union of its
 * intervals [start, end); intervals that overlap or touch merge (bedtools merge, distance 0).  An interval belongs to
 * (group[i], seq[i]); 0 <= start <= end < 2^32. */
int mpn_cover_by_group(int64_t n, const int32_t *group, const int32_t *seq, const int64_t *start, const int64_t *end,
                       int32_t n_groups, int64_t *covered);

/* Events that one block of the depth sweep scans (a multiple of its 256 lanes); block partials are carried between such tiles. */
#define MPN_DEPTH_TILE 2048

/* Depth profile, depth BED and depth span of n intervals [start, end), 0 <= start, end < 2^32.  Interval i lies on key[i] in
 * [0, n_keys): one (assembly, sequence) pair of length key_len[k] < 2^32 that belongs to group key_group[k] in [0, n_groups).
 *   - an interval with start >= end or start >= key_len contributes nothing; an end beyond key_len is clipped to key_len;
 *   - the depth of a position is the number of contributing intervals that cover it;
 *   - profile: the maximal runs of constant non-zero depth of every key, ordered by (key, start) -- book-ended intervals do
 *     not split a row;
 *   - a row of group g passes iff depth_lo[g] <= depth <= depth_hi[g] (both NULL: every row passes);
 *   - BED: the passing rows, rows of one key that touch merged, ordered by (key, start);
 *   - span[g] (zeroed by the call): the summed length of the passing rows of group g.
 * cap: the capacity of each output list, >= 2n when the profile or the BED is wanted.  The four row_* pointers and n_rows are
 * all NULL (profile not wanted) or all given; likewise the three bed_* pointers and n_bed; span may be NULL.  n < 2^30.
 * A record outside the domain or a cap below 2n returns -2 before anything is written. */
int mpn_depth_by_key(int64_t n, const int32_t *key, const int64_t *start, const int64_t *end,
                     int32_t n_keys, const int64_t *key_len, const int32_t *key_group,
                     int32_t n_groups, const int32_t *depth_lo, const int32_t *depth_hi,
                     int64_t cap,
                     int32_t *row_key, int64_t *row_start, int64_t *row_end, int32_t *row_depth, int64_t *n_rows,
                     int32_t *bed_key, int64_t *bed_start, int64_t *bed_end, int64_t *n_bed,
                     int64_t *span);

/* Records that one block of the union sweep scans (a multiple of its 256 lanes); the running maximum of `end`, the count of
 * merged intervals and their summed length are carried between such tiles. */
#define MPN_BED_TILE 2048

/* The union of n intervals [start, end), 0 <= start, end < 2^32, per key[i] in [0, n_keys): intervals of one key that overlap
 * or touch merge (bedtools merge, distance 0); an interval with start >= end contributes nothing.  The merged intervals come
 * out ordered by (key, start) in out_key / out_start / out_end[0..*n_out), cap >= n entries each; span[g] (g < n_groups, zeroed
 * by the call, may be NULL) = their summed length over the keys with key_group[k] == g.  n < 2^31.
 * A record or key_group outside the domain or a cap below n returns -2 before anything is written. */
int mpn_bed_union(int64_t n, const int32_t *key, const int64_t *start, const int64_t *end,
                  int32_t n_keys, const int32_t *key_group, int32_t n_groups,
                  int64_t cap, int32_t *out_key, int64_t *out_start, int64_t *out_end, int64_t *n_out, int64_t *span);

/* covered[i], i < n_q = the number of positions of the query interval [q_start[i], q_end[i]) on q_key[i] that at least one of
 * the n_bed BED intervals of the same key covers (both keyed into [0, n_keys)).  A BED interval counts through its clip to the
 * query, max of the starts to min of the ends, and only where that is not empty: one that merely touches the query, or is
 * itself empty (start >= end), adds nothing.  0 <= q_start <= q_end < 2^32; a query with q_start == q_end gets 0; BED records as
 * in mpn_bed_union.  The BED is merged on the device and stays there; only covered[] comes back.
 * A record outside the domain (a query with q_start > q_end included) returns -2 before anything is written. */
int mpn_cover_by_bed(int64_t n_bed, const int32_t *bed_key, const int64_t *bed_start, const int64_t *bed_end,
                     int64_t n_q, const int32_t *q_key, const int64_t *q_start, const int64_t *q_end,
                     int32_t n_keys, int64_t *covered);

/* Rows that one block of the best-alignment scans covers (a multiple of its 256 lanes); the running arg-max, maximum, count and
 * sum are carried between such tiles, so a read or a (read, assembly) group may run through any number of them. */
#define MPN_BEST_TILE 2048

/* The candidates of every read for its best alignment (the reference's bin/megapath_nano.py:250-273, the part of
 * align_list_to_best_align_list before the abundance).  Row i is an alignment of read[i] in [0, n_reads) on assembly[i] in
 * [0, n_assemblies) with score[i] (any int64 but the smallest one) and tiebreak[i] (a finite double; -0.0 counts as 0.0).
 *   - per (read, assembly) the row with the largest (score, tiebreak) is kept, the LAST in input order among equal ones;
 *   - a kept row is a candidate iff its score equals the largest score of its read: one candidate per assembly at most.
 * cand_row / cand_read[0..*n_cand), room for n entries each: the candidates' row indices and read codes, ordered by (read,
 * assembly).  read_count[r] / read_first[r], r < n_reads: the number of candidates of read r and the position of its first one in
 * that list (a read without rows has count 0 and the position where its candidates would stand).  n < 2^31.
 * A record outside the domain returns -2 before anything is written. */
int mpn_best_candidates(int64_t n, const int32_t *read, const int32_t *assembly, const int64_t *score, const double *tiebreak,
                        int32_t n_reads, int32_t n_assemblies,
                        int64_t *cand_row, int32_t *cand_read, int64_t *n_cand, int64_t *read_count, int64_t *read_first);

/* The abundance-weighted draw among the candidates of every read (bin/megapath_nano.py:283-310).  Candidate j < m belongs to
 * read[j] in [0, n_reads), non-decreasing in j, has weight[j] >= 0 (the abundance of its assembly; the weights of one read sum to
 * less than 2^53), its own tiebreak[j] and the random number draw[j], both finite.  With s = the summed weight of the read:
 *   - a read with ONE candidate keeps it: new_tiebreak[j] = tiebreak[j], draw[j] is not looked at;
 *   - otherwise new_tiebreak[j] = draw[j] * (s <= 0 ? 1.0 : (double)weight[j] / (double)s): one IEEE float64 division and one
 *     multiplication (the conversions are exact in this domain), and tiebreak[j] is not looked at;
 *   - winner[r], r < n_reads = the candidate of read r with the largest new_tiebreak, the LAST one among equal ones; -1 for a read
 *     without candidates.  (The candidates of a read share one score, so the score plays no part here.)
 * m < 2^31.  A record outside the domain returns -2 before anything is written. */
int mpn_pick_weighted(int64_t m, const int32_t *read, const int64_t *weight, const double *tiebreak, const double *draw,
                      int32_t n_reads, double *new_tiebreak, int64_t *winner);

/* second[r], r < n_reads = the largest score[i] over the rows with read[i] == r and assembly[i] != excluded[r], or 0 if there is
 * no such row (the reference's step_unique_alignment, bin/megapath_nano.py:2563-2584, where a missing second best is filled
 * with 0).  read[i] in [0, n_reads); assembly[i] >= 0; excluded[r] is an assembly code or -1 (nothing excluded); score[i] is any
 * int64 but the smallest one.  A record outside the domain returns -2 before anything is written. */
int mpn_second_best_by_read(int64_t n, const int32_t *read, const int32_t *assembly, const int64_t *score,
                            int32_t n_reads, const int32_t *excluded, int64_t *second);

/* The good alignments of every read (the reference's good_align_list, bin/megapath_nano.py:642-663; with one unit and no threshold
 * the `sort_values(read, score, tiebreaker).drop_duplicates(read, keep='last')` of :1287 and :1459).  Row i is an alignment of
 * read[i] in [0, n_reads) on unit[i] in [0, n_units) -- an assembly, a sequence, or the single unit 0 -- with |score[i]| < 2^53 and
 * a finite tiebreak[i] (-0.0 counts as 0.0).
 *   - per (read, unit) the row with the largest (score, tiebreak) is kept, the LAST in input order among equal ones;
 *   - read_best[r], r < n_reads = the largest kept score of read r, 0 for a read without rows;
 *   - a kept row is good iff use_threshold == 0 or (double)score >= (double)read_best * threshold: ONE IEEE float64 product (both
 *     conversions are exact in this domain), as pandas evaluates `alignment_score >= best_alignment_score * pct`.
 * good_row[0..*n_good), room for n entries: the good rows' indices, ordered by (read, unit).  n < 2^31; threshold is finite (it is
 * checked whether or not it is used).  Bad arguments or a record outside the domain return -2 before anything is written or
 * launched. */
int mpn_good_rows(int64_t n, const int32_t *read, const int32_t *unit, const int64_t *score, const double *tiebreak,
                  int32_t n_reads, int32_t n_units, int32_t use_threshold, double threshold,
                  int64_t *good_row, int64_t *n_good, int64_t *read_best);

/* The grouped sums of the reference's summary_stat_1 (bin/megapath_nano.py:485-493).  cols: n_cols (1..6) arrays of n values, one
 * after another, each |value| < 2^32; row i belongs to key[i] in [0, n_keys).  count[k] = the number of rows of key k;
 * sums[c * n_keys + k] = the sum of column c over them; keys without rows get 0.  n < 2^31, so no sum leaves int64.  A segmented
 * scan over the rows sorted by key: no atomic touches the output, and the cost does not depend on how the rows spread over the keys.
 * Bad arguments or a record outside the domain return -2 before anything is written or launched. */
int mpn_sum_by_key(int64_t n, const int32_t *key, int32_t n_keys, int32_t n_cols, const int64_t *cols,
                   int64_t *count, int64_t *sums);

#ifdef __cplusplus
}
#endif
#endif
