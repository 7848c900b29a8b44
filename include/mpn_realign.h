/*
 * mpn_realign.h -- C-ABI of the MI355X-native amplicon realigner (libmpn.so), SURVEY.md section 8 row f4.
 *
 * Part 1 is the drop-in boundary: the two symbols the reference binds with ctypes in
 *   /root/reference/bin/realignment/realign_illumina_reads.py:40-43 (struct), :596-605 (realign_reads), :627-629 (free_memory)
 * with the prototypes of
 *   /root/reference/bin/realignment/realign/realigner.cpp:854-869 and the struct of realigner.h:42-46.
 * A maintainer switches over by pointing `realigner_mod` (realign_illumina_reads.py:32) at libmpn.so.
 * The k-mer seeded Hamming placement of reads on haplotypes (ReAligner::FastAlignReadsToHaplotypes, realigner.cpp:147-230)
 * and every Smith-Waterman alignment (haplotype -> reference, read -> haplotype; ssw_cpp.cpp:268-300 over ssw.c) run as
 * HIP kernels (csrc/realign.hip, csrc/ssw_kernels.hip).  There is no CPU fallback: on a HIP failure realign_reads
 * prints the error and returns NULL.
 *
 * Part 2 is the batched form the reference does not have (it calls realign_reads once per window from a Python loop,
 * realign_illumina_reads.py:533-629): many windows per call, one launch per stage over all of them.
 *
 * Preconditions (the reference's behaviour is undefined outside them): every haplotype has >= 32 bases, at most 1000
 * reads per window through Part 1 (the reference's fixed arrays), 7-bit ASCII sequences.
 */
#ifndef MPN_REALIGN_H
#define MPN_REALIGN_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Part 1: reference-compatible symbols -------------------------------------------- */
typedef struct {              /* realigner.h:42-46 */
    int position[1000];
    char *cigar_string[1000];
} struct_str_arr;

/* haplotypes: whitespace-separated sequences (realigner.cpp:787-792).  Returns a new struct_str_arr whose first
 * read_size entries are filled (cigar strings individually allocated); release it with free_memory(ptr, read_size). */
struct_str_arr *realign_reads(char *seqs[], int *positions, char *cigars[], char *reference, char *haplotypes,
                              int ref_start, int ref_prefix, int ref_suffix, int read_size);
void free_memory(struct_str_arr *pointer, int size);

/* ---- Part 2: batched form ------------------------------------------------------------- */
typedef struct {
    int32_t n_reads;
    const char *const *seqs;       /* n_reads NUL-terminated reads */
    const int32_t *positions;      /* n_reads */
    const char *const *cigars;     /* n_reads NUL-terminated CIGAR strings (returned unchanged for reads left alone) */
    const char *reference;         /* ref_prefix + window + ref_suffix */
    int32_t n_haps;
    const char *const *haplotypes; /* n_haps NUL-terminated candidate haplotypes */
    int32_t ref_start, ref_prefix, ref_suffix;
} mpn_realign_window;

/* out_position / out_cigar: one entry per read of every window, in window order.  out_cigar[i] is malloc'd; release
 * the whole array's strings with mpn_realign_free_cigars.  Returns 0, or a negative code with mpn_last_error(). */
int mpn_realign_batch(int32_t n_windows, const mpn_realign_window *windows, int32_t *out_position, char **out_cigar);
void mpn_realign_free_cigars(char **cigars, int64_t n);

/* ---- Part 3: stage entry of the placement stage (for the parity tests) ------------------ */
/* One accepted placement of a read on a haplotype (hap and read count inside their window): the read fits at `start` with `mm`
 * (<= 2) mismatches, and the reference's loop would first have evaluated it at haplotype position `t` through the read's k-mer at
 * offset `p` (start == max(0, t - p)). */
typedef struct {
    int32_t window, hap, read, start, mm, t, p;
} mpn_realign_hit;

/* Runs the two steps mpn_realign_batch begins with -- the placement kernel over every (haplotype, read) pair, then the
 * per-haplotype bookkeeping of FastAlignReadsToHaplotypes (realigner.cpp:147-230) -- on the same windows, and returns what they
 * leave before any Smith-Waterman step (tests/test_realign_place_gpu.py; positions, cigars, ref_start and the content of
 * reference beyond its comparison with the haplotypes are not read).
 *   list_cap   capacity of the first launch's hit list, grid_cap the largest grid; 0: the realigner's own value
 *   hit_cap    room in out_hits; at least the sum over the pairs of max(0, haplotype length - read length + 1) is asked for
 *   out_hits   the hits in the reference's order of evaluation (haplotype, t, read, p); *out_n_hits of them
 *   out_kmer   per haplotype, one byte per position 0 .. length - 32: 1 where the 32-mer there is a k-mer of any read of the
 *              window longer than 32 bases (the haplotypes of all windows in order, back to back)
 *   out_dropped, out_hap_score   per haplotype: 1 where the coverage test ended it (:224-228), and its score
 *   out_position, out_score      per (haplotype, read) in window, haplotype, read order: -1 / 0 where the read is not placed
 *   out_launches  kernel launches it took: 2 when the first list overflowed (a second overflow is an error, -1)
 * Malformed windows, haplotypes under 32 bases, negative knobs and a hit_cap too small are refused before anything is uploaded
 * (-2, mpn_last_error()); the outputs are written only on success. */
int mpn_realign_place_batch(int32_t n_windows, const mpn_realign_window *windows, int64_t list_cap, int32_t grid_cap,
                            int64_t hit_cap, mpn_realign_hit *out_hits, int64_t *out_n_hits, uint8_t *out_kmer,
                            uint8_t *out_dropped, int32_t *out_hap_score, int32_t *out_position, int32_t *out_score,
                            int32_t *out_launches);

#ifdef __cplusplus
}
#endif
#endif
