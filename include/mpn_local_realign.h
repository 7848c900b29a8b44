/*
 * mpn_local_realign.h -- C-ABI of the local realignment around called variants on the GPU (csrc/local_realign_kernels.hip), the
 * drop-in for realignment/local_realignment.py -p ont of the reference (megapath_nano_amd/local_realign.py; the rules are DESIGN.md
 * section 6 item 20).  The BAM text is resident, as for mpn_tensor.h and mpn_call.h.
 *
 *   mpn_lr_depth_rule    host only: which candidates of a deep site samtools' -d 8000 keeps
 *   mpn_lr_columns       accepted (site, read) pairs -> the surviving columns of every site, 401 bits a site, in HBM
 *   mpn_lr_fragments     pairs and columns -> what every read appends over its site's columns: lengths, then bytes, in HBM
 *   mpn_lr_align_tally   resident fragments -> SSW against every site's reference window, the allele of every read at its site, and
 *                        per site the ordered (key, count) list, a CSR in HBM
 *   mpn_ssw_align_resident   the SSW of mpn_ssw_align_batch on reads and references that are in HBM already (a stage entry)
 *
 * The arithmetic shared by host and device is csrc/local_realign_core.h (scripts/local_realign_host_check.cpp runs it serially).
 * Calling rules as in mpn_tensor.h: a call returns when its results are in place, the default stream is used, 0 = done, -1 = device
 * error (mpn_last_error()), -2 = bad arguments, -3 = an output does not fit.  Malformed records end in *bad_pair, never in an access
 * outside the text.
 */
#ifndef MPN_LOCAL_REALIGN_H
#define MPN_LOCAL_REALIGN_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPN_LR_WINDOW 200            /* realign_windows: the columns pos - 200 .. pos + 200 */
#define MPN_LR_REGION 233            /* the pile-up region is pos - 233 .. pos + 234 */
#define MPN_LR_FLANK 300             /* the reference window is contig[pos - 301 : pos + 300] */
#define MPN_LR_COLUMNS 401
#define MPN_LR_MASK_WORDS 13         /* uint32 words of a site's column mask */
#define MPN_LR_MAXCNT 8000           /* samtools mpileup's default -d */
#define MPN_LR_REF_STRIDE 608        /* bytes between the reference windows of two sites */
#define MPN_LR_MAX_KEYS 4            /* allele keys of one read at its site, at the most */

/* why a pair is refused */
#define MPN_LR_OK 0
#define MPN_LR_PAST 1                /* the record, its CIGAR or its bases pass the end of the record or the text */
#define MPN_LR_BAD_OP 2              /* an operation code above 8 at or before the site's region */
#define MPN_LR_SKIP_PAD 3            /* an N or P operation inside the site's region */
#define MPN_LR_NO_BASES 4            /* a record without bases */
#define MPN_LR_EQ_BASE 5             /* a base `=` under a column or in an insertion of the window */
#define MPN_LR_PAST_BASES 6          /* the CIGAR runs past the bases */

/* A record that mpileup would take (flags, contig), in file order.  pos: 0-based. */
typedef struct {
    int64_t off;
    int32_t pos;
    int32_t reserved;
} mpn_lr_read;

/* An accepted record of a site: indices into the call's sites and reads.  Pairs are sorted by site, then by read. */
typedef struct {
    int32_t site;
    int32_t read;
} mpn_lr_pair;

/* One distinct allele key of a site: its count, and its text at bytes[off .. off + len). */
typedef struct {
    int32_t count;
    int32_t len;
    int64_t off;
} mpn_lr_key;

/* keep[i] = 1 iff candidate i (start[i] ascending, end[i] exclusive, htslib's bam_endpos) is piled up: it is the first candidate of
 * its start, or fewer than maxcnt kept candidates have end >= start[i]. */
int32_t mpn_lr_depth_rule(int64_t n, const int64_t *start, const int64_t *end, int32_t maxcnt, uint8_t *keep);

/* d_mask (DEVICE, m * MPN_LR_MASK_WORDS uint32): bit d of site c is set iff column site_pos[c] - 200 + d survives: an accepted read
 * covers it (M, =, X or D), none has a matched base there that is not one of ACGTN (the script drops such a row), and no column
 * between the centre and it is missing.  site_pos: host, 1-based.  *bad_pair: -1 or the smallest refused pair, *bad_why: its reason.
 * An operation code above 8 is looked for from the record's first operation to the end of the 64-operation step that passes the
 * region (the serial form stops at the operation that passes it).
 * hazards (host, 3 * hazard_cap int64: pair, 0-based column, raises; any order): where a matched stretch ends inside the region on
 * a base that is not one of ACGTN, directly followed by an I or a D.  raises = 1 iff no earlier pair of the site gives the script's
 * parser an entry at that column (a deleted base or a matched one of ACGTN): the script raises IndexError there and the site has no
 * line.  Pairs are sorted by site, then by read.  *n_hazards = their number; -3 if it is more than hazard_cap (call again with room). */
int32_t mpn_lr_columns(const void *d_text, int64_t text_len, int64_t n_reads, const mpn_lr_read *reads, int64_t m, const int32_t *site_pos,
                       int64_t n_pairs, const mpn_lr_pair *pairs, void *d_mask, int64_t *bad_pair, int32_t *bad_why, int64_t *hazards,
                       int64_t hazard_cap, int64_t *n_hazards);

/* A wave per pair.  d_letters == NULL: len[i] (host) = the bytes pair i appends, first[i] (host) = the 0-based reference position of
 * the first column at which it appends (undefined for len 0).  Otherwise the bytes of pair i go to d_letters[frag_off[i] ..] (DEVICE,
 * cap bytes; upper-case letters) and their SSW codes (A C G T -> 0 1 2 3, any other 4) to d_codes at the same place; a pair with
 * frag_off[i] < 0 is passed over. */
int32_t mpn_lr_fragments(const void *d_text, int64_t text_len, int64_t n_reads, const mpn_lr_read *reads, int64_t m, const int32_t *site_pos,
                         int64_t n_pairs, const mpn_lr_pair *pairs, const void *d_mask, int32_t *len, int32_t *first, const int64_t *frag_off,
                         void *d_letters, void *d_codes, int64_t cap, int64_t *bad_pair, int32_t *bad_why);

/* The pairs of site c are pair_begin[c] .. pair_begin[c + 1] (host), in the order of the script's dict; pair i's fragment is
 * frag_len[i] > 0 bytes at frag_off[i] of d_letters / d_codes (DEVICE).  d_contig: the contig_len bytes of the contig (DEVICE), 300 <
 * site_pos[c] <= contig_len.  Every fragment is aligned as pyssw.SSW.align does it against the site's window.  Results (host):
 * depth[c]; raises[c] = 1 iff the site's first read has score 0 (the script raises there; the site has no keys); key_begin[c] ..
 * key_begin[c + 1] = the site's entries of d_keys (DEVICE, mpn_lr_key, keys_cap entries) in the order of first insertion, their text in
 * d_bytes (DEVICE, bytes_cap).  *bad_pair: -1, or the smallest pair with a positive score that SSW refuses (*bad_why: its status). */
int32_t mpn_lr_align_tally(int64_t m, const int32_t *site_pos, const int64_t *pair_begin, int64_t n_pairs, const int64_t *frag_off,
                           const int32_t *frag_len, const void *d_letters, const void *d_codes, const void *d_contig, int64_t contig_len,
                           int32_t *depth, int32_t *raises, int64_t *key_begin, void *d_keys, int64_t keys_cap, void *d_bytes, int64_t bytes_cap,
                           int64_t *bad_pair, int32_t *bad_why);

/* mpn_ssw_align_batch with d_reads and d_refs on the DEVICE.  d_res (DEVICE, 9 * n_pairs int32): the rows score1, score2, ref_begin1,
 * ref_end1, read_begin1, read_end1, ref_end2, status, need_cigar.  d_cigar (DEVICE, cigar_cap uint32): pair i's operations at
 * cigar_off[i] .. + cigar_len[i] (host).  status: host.  -3 if the CIGARs need more than cigar_cap entries. */
int32_t mpn_ssw_align_resident(int32_t n_pairs, const void *d_reads, const int64_t *read_off, const int32_t *read_len, const void *d_refs,
                               const int64_t *ref_off, const int32_t *ref_len, const int8_t *mat, int32_t n, int8_t score_size, uint8_t gap_open,
                               uint8_t gap_extend, uint8_t flag, uint16_t filters, int32_t filterd, const int32_t *mask_len, void *d_res,
                               void *d_cigar, int64_t cigar_cap, int64_t *cigar_off, int32_t *cigar_len, int32_t *status);

/* Device time of the calling thread's last call of columns, fragments, and of align_tally's SSW and tally, in milliseconds. */
void mpn_lr_last_device_ms(double *columns_ms, double *fragments_ms, double *ssw_ms, double *tally_ms);

#ifdef __cplusplus
}
#endif
#endif
