/*
 * mpn_call.h -- C-ABI of the decoding of Clair's probabilities into VCF records on the GPU (csrc/clair_call_kernels.hip), the
 * drop-in for output_from / output_with of clair/call_var.py and its pysam look-ups (megapath_nano_amd/clair_call.py; the rules
 * are DESIGN.md section 6 item 19).  The BAM text is resident, as for mpn_tensor.h.
 *
 *   mpn_call_indels    taken records and sorted sites -> the distinct indel events of every site's pile-up column, a CSR list in HBM
 *   mpn_call_decode    probabilities, tensors, reference strings and events -> the compact rows of the sites that give a record
 *   mpn_call_quantize  probabilities -> what the text round trip through %.6f leaves of them
 *
 * The arithmetic shared by host and device is csrc/clair_call_core.h (scripts/clair_call_host_check.cpp runs it serially).  Calling
 * rules as in mpn_tensor.h: a call returns when its results are in place, the default stream is used, 0 = done, -1 = device error
 * (mpn_last_error()), -2 = bad arguments.  Malformed records end in *bad_read, never in an access outside the text.
 */
#ifndef MPN_CALL_H
#define MPN_CALL_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPN_CALL_MAX_LEN 50          /* maximum_variant_length_that_need_infer: longer events can never be selected */
#define MPN_CALL_MAX_DEPTH 250       /* max_depth of the pile-up */
#define MPN_CALL_MAX_EVENTS 256      /* distinct events of one site at the most */
#define MPN_CALL_PROBS 90            /* gt21 (21) | genotype (3) | length_1 (33) | length_2 (33) */
#define MPN_CALL_REF 33              /* bytes of a site's reference string */
#define MPN_CALL_ALLELE_BYTES 256    /* a row's alleles: REF at 0 (<= 51), the first ALT at 51 (<= 101), the second at 152 (<= 101) */
#define MPN_CALL_ALT1_AT 51
#define MPN_CALL_ALT2_AT 152

#define MPN_CALL_INSERTION 0
#define MPN_CALL_DELETION 1

/* options of mpn_call_decode */
#define MPN_CALL_PYSAM_ALL 1         /* --pysam_for_all_indel_bases */
#define MPN_CALL_HAPLOID 2           /* --haploid */
#define MPN_CALL_SHOW_REF 4          /* --showRef */

/* what became of a site */
#define MPN_CALL_EMITTED 0
#define MPN_CALL_NOT_ACGT 1          /* the centre base is not one of ACGTU */
#define MPN_CALL_NO_DEPTH 2          /* read depth 0 */
#define MPN_CALL_REFERENCE 3         /* a reference call that is not shown */
#define MPN_CALL_SAME 4              /* REF == ALT */
#define MPN_CALL_RAISES 5            /* the reference script raises here (a centre U in a heterozygous call) */
#define MPN_CALL_BAD_PROB 6          /* a probability that is NaN, negative or infinite: refused */
#define MPN_CALL_LONG_KEY 7          /* the chosen insertion has a deletion spelled behind it and the text is longer than 50 bytes */

/* A record that passes the flag filter and lies on the contig, in file order.  rlen: htslib's bam_cigar2rlen (M, D, N, = and X). */
typedef struct {
    int64_t off;
    int64_t rlen;
    int32_t pos;
    int32_t reverse;       /* FLAG & 16 */
} mpn_call_read;

/* One distinct event of a site.  len: the number the pile-up spells (inserted bases and pads; deleted bases).  count: the reads
 * of the column that show it.  rank: the place in the column of the first of them.  clip: for a deletion, len clipped at the end
 * of the contig; for an insertion, the length of the deletion right behind it (0: none), which pileup_seq spells into the same text
 * (`+2AA-3NNN`), so that the script takes `AA-3NNN` for the inserted bases.  key_len: the bytes of the key the script counts: clip
 * for a deletion; for an insertion len, or len + 1 + digits + clip with such a deletion, or -1 if that is more than
 * MPN_CALL_MAX_LEN (the arena then holds the len bases only).  bases: for an insertion, the offset of the key's bytes in the arena. */
typedef struct {
    int32_t kind;
    int32_t len;
    int32_t count;
    int32_t rank;
    int32_t clip;
    int32_t key_len;
    int64_t bases;
} mpn_call_event;

/* The events of m sites (site[c]: host, 1-based positions, strictly ascending) over the reads begin[c] .. end[c] (host; the caller
 * bisects them).  The column of a site is what AlignmentFile.pileup(start=site, stop=site+1, max_depth=250) holds at the 0-based
 * position site - 1: of the reads that overlap the 0-based base `site`, the first 250 and the first of every start position.
 * d_events == NULL: counts[c] (host) = the distinct events.  Otherwise entry i of site c is written to
 * ((mpn_call_event *)d_events)[ev_off[c] + i] (DEVICE, events_cap entries; ev_off: host, the running sum of the counts) in the
 * order of first appearance, its bases to ((uint8_t *)d_bases)[(ev_off[c] + i) * MPN_CALL_MAX_LEN ..] (DEVICE), and counts is
 * filled again.  A wave per site.  *bad_read: -1, or the smallest index of a read of a column that does not lie inside the text,
 * has an operation code above 8 or an inserted base past its bases.  *bad_site: -1, or the smallest site with more than
 * MPN_CALL_MAX_EVENTS distinct events.  The events are not to be used then. */
int32_t mpn_call_indels(const void *d_text, int64_t text_len, int64_t n_reads, const mpn_call_read *reads, int64_t m, const int32_t *site,
                        const int64_t *begin, const int64_t *end, int64_t contig_len, int64_t *counts, const int64_t *ev_off, void *d_events,
                        void *d_bases, int64_t events_cap, int64_t *bad_read, int64_t *bad_site);

/* A record of the VCF before its text: the site (index into the call's sites), the ten flags of output_from (bit 0: reference,
 * 1: homo SNP, 2: hetero SNP, 3: homo insertion, 4: hetero ACGT + insertion, 5: two insertions, 6: homo deletion, 7: hetero ACGT +
 * deletion, 8: two deletions, 9: insertion and deletion), the genotype (0: 0/0, 1: 1/1, 2: 0/1, 3: 1/2), the indices into the
 * gt21 and genotype probabilities, their float32 product p, and the lengths of the alleles (alt2_len 0: one ALT). */
typedef struct {
    int32_t site;
    int32_t flags;
    int32_t genotype;
    int32_t gt21;
    int32_t genotype_task;
    float p;
    int32_t supported;
    int32_t depth;
    int32_t ref_len;
    int32_t alt1_len;
    int32_t alt2_len;
    int32_t reserved;
} mpn_call_row;

/* Decodes m sites, a wave per site.  DEVICE: d_probs (float32, 90 per site), d_tensors (int32, 1056 per site), d_refs (33 bytes
 * per site, of which ref_n[c] (host, 17 .. 33) count), d_contig (the contig_len bytes of the contig, for the deleted bases),
 * d_events / d_bases (n_events entries, as mpn_call_indels leaves them; the events of site c are ev_begin[c] .. ev_end[c]: host, so
 * that several tensors of one position share a list).  site: host, 1-based.
 * status[c] (host) = what became of site c.  The rows of the emitted sites are written in site order to d_rows
 * (mpn_call_row) and d_alleles (MPN_CALL_ALLELE_BYTES each), both DEVICE with room for m; *n_rows = their number. */
int32_t mpn_call_decode(int64_t m, const int32_t *site, const void *d_probs, const void *d_tensors, const void *d_refs, const int32_t *ref_n,
                        const void *d_contig, int64_t contig_len, const int64_t *ev_begin, const int64_t *ev_end, const void *d_events,
                        const void *d_bases, int64_t n_events, int32_t options, int32_t *status, void *d_rows, void *d_alleles, int64_t *n_rows);

/* d_probs[i] (DEVICE, float32, n values) = float32(rint(double(p) * 1e6) / 1e6): what `%.6f` and a float32 parse leave of p. */
int32_t mpn_call_quantize(void *d_probs, int64_t n);

/* Device time of the calling thread's last call of indels, decode and quantize, in milliseconds.  Any pointer may be NULL. */
void mpn_call_last_device_ms(double *indels_ms, double *decode_ms, double *quantize_ms);

#ifdef __cplusplus
}
#endif
#endif
