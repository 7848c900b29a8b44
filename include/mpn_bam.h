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

#ifdef __cplusplus
}
#endif
#endif
