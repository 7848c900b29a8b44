/*
 * mpn_bam.h -- C-ABI of the native halves of the BAM writer, the work of `samtools view -b | samtools
 * sort` in the pipeline the reference starts after the species placement (/root/reference/bin/lib/aligner.py:246-252):
 *
 *   mpn_bam_encode      SAM lines -> BAM records (SAMv1 section 4.2 as htslib 1.13 writes them: sam.c sam_parse1 / bam_write1).
 *                       Host code, multi-threaded over the lines of a batch.
 *   mpn_bgzf_compress   payload blocks -> complete BGZF blocks (SAMv1 section 4.1: gzip member header with the BC field, one raw
 *                       deflate stream, CRC32, ISIZE), deflated on the GPU, one workgroup per block (csrc/bgzf_kernels.hip).
 *
 * BGZF blocking, the coordinate sort (mpn_sort_order), the BAI index and the default zlib compression stay in
 * megapath_nano_amd/bam.py, which the reference's vendored htslib test data pin (tests/golden/htslib); bam.py hands its blocks to
 * mpn_bgzf_compress only when asked to (compress_blocks=bam.device_bgzf_blocks, MPN_BGZF=device).
 *
 * The device writer (opt-in: bam.sam_to_sorted_bam_device, MPN_BAM_WRITER=device, bin/mpn-sam2bam) keeps the records on the device
 * between the SAM text and the deflate (csrc/bam_out_kernels.hip, csrc/bam_out_core.h):
 *
 *   mpn_bam_out_*          SAM text in, batch by batch -> <out>.bam and <out>.bam.bai, byte for byte what bam.sam_to_sorted_bam
 *                          writes with the device sort and the device deflate.  Line starts, the scan of every line (tabs, FLAG,
 *                          refID, POS, record size, status), the encode into a resident record pool, the gather of the sorted
 *                          records into block payloads and the deflate are kernels; the coordinate sort is mpn_sort_order; the
 *                          block cut and the index are serial host code (a few bytes per record are downloaded for them).
 *   mpn_sam_encode_batch   scan + encode of given lines through the same launches, for tests.
 *   mpn_bai_build          bam.BaiBuilder in C++: records in file order with their virtual offsets -> the bytes of the .bai.
 *
 * A line is encoded exactly as mpn_bam_encode encodes it or it is REFUSED with one of the MPN_SAM_* statuses below; the writer then
 * writes nothing, and the caller takes the host path.
 */
#ifndef MPN_BAM_H
#define MPN_BAM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpn_bam_encoder mpn_bam_encoder;

/* an encoder for the references of one SAM header (@SQ order): RNAME / RNEXT -> refID */
mpn_bam_encoder *mpn_bam_encoder_create(const char *const *ref_names, int32_t n_ref);
void mpn_bam_encoder_destroy(mpn_bam_encoder *e);

/* n SAM lines: line i is text[line_off[i] .. line_off[i] + line_len[i]) (a trailing newline is ignored).  Record i (WITHOUT its
 * block_size word) goes to out[rec_off[i] .. rec_off[i + 1]); tid / pos0 / end0 / flag [i] receive what the index builder needs
 * (end0 = pos0 + reference length of the CIGAR, pos0 + 1 for a record without one or an unmapped one).  A CIGAR of more than
 * 65535 operations travels as <l_seq>S<ref_len>N + a CG:B,I tag (htslib bam_write1).  Returns the bytes written, -3 if out_cap is
 * too small (nothing usable is left in out), or -1 (mpn_last_error(): malformed line, unknown tag type, integer out of range). */
int64_t mpn_bam_encode(const mpn_bam_encoder *e, const char *text, const int64_t *line_off, const int32_t *line_len, int64_t n,
                       uint8_t *out, int64_t out_cap, int64_t *rec_off, int32_t *tid, int32_t *pos0, int32_t *end0, int32_t *flag);

/* How mpn_bgzf_compress forms the deflate stream of every block.  AUTO: LZ77 matches + dynamic Huffman codes, or the stored form
 * where that is not larger.  STORED: always the stored form.  NO_MATCH: literals only (dynamic Huffman codes, or stored where that
 * is not larger).  The last two exist so that each half can be tested alone. */
enum { MPN_BGZF_AUTO = 0, MPN_BGZF_STORED = 1, MPN_BGZF_NO_MATCH = 2 };

/* n_blocks payloads: block i is payload[pay_off[i] .. pay_off[i + 1]), 0..65280 bytes.  out receives the complete BGZF blocks one
 * after another: the 18-byte header with BSIZE, ONE raw deflate stream (BFINAL = 1; BTYPE 2 with HLIT >= 257, HDIST >= 1,
 * HCLEN >= 4, complete codes of at most 15 / 15 / 7 bits, or BTYPE 0), CRC32 and ISIZE; block i is out[out_off[i] .. out_off[i + 1]).
 * A block is never larger than its stored form (payload + 31 bytes, so BSIZE <= 65310), and its bytes depend on its payload and
 * the mode alone, not on its place in the batch.  Calling rules as for mpn_sort_order: all pointers are HOST pointers, the call
 * returns when the result is in out, the default stream is used.
 * Returns the total number of bytes; -3 if out_cap is too small (out_off is complete, out_off[n_blocks] is the size needed, out is
 * not written); -1 (mpn_last_error()) for a block longer than 65280 bytes or of negative length -- before anything is launched --
 * and for a device error; -2 for bad arguments. */
int64_t mpn_bgzf_compress(int64_t n_blocks, const uint8_t *payload, const int64_t *pay_off /* n + 1 */,
                          uint8_t *out, int64_t out_cap, int64_t *out_off /* n + 1 */, int32_t mode);

/* Device time of the calling thread's last mpn_bgzf_compress by HIP events, in milliseconds: the deflate launches with the
 * address scan, and the packing kernel (0 where a call ended before them).  Either pointer may be NULL. */
void mpn_bgzf_last_device_ms(double *deflate_ms, double *pack_ms);

/* ---- the device writer ---------------------------------------------------------------------------------------------------------- */

/* What the scan says about a line.  The first three are no faults; every other one is a refusal.  A line with several faults
 * reports the one with the smallest code. */
enum {
    MPN_SAM_OK = 0,
    MPN_SAM_SKIPPED = 1,      /* a header line (@; flag[i] is 1) or a line that is empty after stripping white space: no record */
    MPN_SAM_EXCLUDED = 2,     /* FLAG has one of exclude_flags: no record */
    MPN_SAM_FEW_FIELDS = 3,   /* fewer than 11 fields */
    MPN_SAM_NOT_NUMBER = 4,   /* FLAG, POS, MAPQ, PNEXT or TLEN is not -?[0-9]+ */
    MPN_SAM_NUM_RANGE = 5,    /* FLAG outside 0..65535, MAPQ outside 0..255, POS outside 0..2^31-1 (a negative POS has no sort key),
                                 PNEXT - 1 or TLEN outside int32, an alignment that ends behind 2^29 (the binning scheme's end), a
                                 record of more than 2^31-1 bytes */
    MPN_SAM_QNAME_LONG = 6,   /* QNAME of more than 254 bytes */
    MPN_SAM_CIGAR_OP = 7,     /* a CIGAR letter outside MIDNSHP=X */
    MPN_SAM_CIGAR_NUM = 8,    /* an operation without a number or above 2^28-1; digits behind the last operation; for a CIGAR of more
                                 than 65535 operations, an l_seq or a reference length above 2^28-1 */
    MPN_SAM_QUAL_LEN = 9,     /* QUAL other than * whose length differs from SEQ's */
    MPN_SAM_TAG_FORM = 10,    /* an optional field shorter than XX:T:, without its colons, or an A field without a value */
    MPN_SAM_TAG_INT = 11,     /* an i value that is not -?[0-9]+ or outside int32 U uint32 */
    MPN_SAM_TAG_FLOAT = 12,   /* an f value outside the forms -?digits and -?digits.digits with at most 15 significant digits and
                                 at most 22 digits behind the point (there (float)((double)m / 10^d) is exactly (float)strtod(text)) */
    MPN_SAM_TAG_ARRAY = 13,   /* a B array */
    MPN_SAM_TAG_TYPE = 14,    /* an unknown tag type */
    MPN_SAM_CR = 15,          /* a carriage return anywhere in the line */
    MPN_SAM_POOL = 16,        /* (the writer only) the record pool would pass pool_bytes */
    MPN_SAM_LATE_HEADER = 17, /* (the writer only) a header line behind a record: the header was complete before the text came */
    MPN_SAM_N_STATUS = 18
};
const char *mpn_sam_status_text(int32_t status);

/* Scan + encode of n lines through the writer's launches; mpn_bam_encode's conventions (HOST pointers, line i is
 * text[line_off[i] .. line_off[i] + line_len[i]), one trailing line feed is ignored, record i WITHOUT its block_size word goes to
 * out[rec_off[i] .. rec_off[i + 1])).  status[i] is an MPN_SAM_* code; a line whose status is not MPN_SAM_OK has no bytes, and its
 * tid / pos0 / end0 / flag are not defined.  Returns the bytes written, -3 if out_cap is too small (rec_off and status are
 * complete, out is not written), -2 for bad arguments, -1 for a device error (mpn_last_error()). */
int64_t mpn_sam_encode_batch(const char *const *ref_names, int32_t n_ref, const char *text, const int64_t *line_off, const int32_t *line_len,
                             int64_t n, int32_t exclude_flags, uint8_t *out, int64_t out_cap, int64_t *rec_off, int32_t *tid, int32_t *pos0,
                             int32_t *end0, int32_t *flag, int32_t *status);

/* bam.BaiBuilder (htslib's hts_idx_push / hts_idx_finish, min_shift 14, 5 levels: bins with less than 64 KiB of compressed span folded
 * into their parents, chunks that touch merged, the pseudo-bin 37450, n_no_coor) over n records in file order: coordinate sorted,
 * the unplaced ones last.  voff_after[i]: the virtual offset behind record i; voff_first: that of the first record; voff_end: that
 * of the end of the data.  Serial host code.  Returns the bytes of the .bai; -3 if out_cap is too small (the return of a call with
 * out_cap = 0 is -3 and *need receives the size); -2 for bad arguments. */
int64_t mpn_bai_build(int32_t n_ref, int64_t n, const int32_t *tid, const int32_t *pos0, const int32_t *end0, const uint64_t *voff_after,
                      const uint8_t *mapped, uint64_t voff_first, uint64_t voff_end, uint8_t *out, int64_t out_cap, int64_t *need);

typedef struct mpn_bam_out mpn_bam_out;

/* A writer for the references of one SAM header (@SQ order, distinct names).  chunk_bytes: the text goes to the device in chunks of
 * at most that many bytes, each ending with its last whole line (a longer line is taken whole).  pool_bytes: the limit of the
 * resident record pool.  NULL on bad arguments or a device error. */
mpn_bam_out *mpn_bam_out_create(const char *const *ref_names, int32_t n_ref, int32_t exclude_flags, int64_t chunk_bytes, int64_t pool_bytes);
void mpn_bam_out_destroy(mpn_bam_out *w);

/* len more bytes of SAM text (header lines and blank lines are skipped; a line may end in a later call).  0; 1 once a line has been
 * refused (mpn_bam_out_refusal says which; further text is ignored); -1 for a device error. */
int32_t mpn_bam_out_add_text(mpn_bam_out *w, const char *text, int64_t len);

/* 1-based number of the first refused line among all lines given so far and its status; returns 0 if none was refused */
int32_t mpn_bam_out_refusal(const mpn_bam_out *w, int64_t *line_no, int32_t *status);

/* The end of the text (a last line needs no line feed).  header: the BAM header as the file's payload has it (magic, l_text, text,
 * n_ref, the references).  Sorts, cuts, gathers, deflates in rounds of whole blocks, writes bam_path and -- unless bai_path is
 * NULL -- the index.  Returns the number of records; -4 if a line was refused (no file has been opened); -1 for a device or file
 * error.  The writer can only be destroyed afterwards. */
int64_t mpn_bam_out_finish(mpn_bam_out *w, const uint8_t *header, int64_t header_len, const char *bam_path, const char *bai_path);

/* Milliseconds of the writer's stages so far, nine values: text upload, scan (with the line starts), encode, sort, gather, deflate,
 * download, file writes, cut + index.  Upload, sort, download, file writes and cut + index are host clocks around calls that have
 * returned; the others are HIP events. */
void mpn_bam_out_stage_ms(const mpn_bam_out *w, double *ms9);

#ifdef __cplusplus
}
#endif
#endif
