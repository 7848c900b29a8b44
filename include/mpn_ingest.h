/*
 * mpn_ingest.h -- C-ABI of the target ingestion on the GPU (MPN_TARGET_INGEST=device): the files of a target set go from
 * compressed bytes to the concatenated bases mpn_index_build_device (mpn_map.h) reads, without existing as host strings.
 *
 *   mpn_gzip_inflate   many gzip files (RFC 1952 members of RFC 1951 deflate streams) -> their bytes, one wave per file
 *                      (csrc/inflate_kernels.hip; the serial decoder is csrc/inflate_core.h and the CRC-32 arithmetic it shares
 *                      with the BGZF writer csrc/crc32_poly.h, which both also compile for the host).
 *   mpn_fasta_scan     FASTA text in HBM -> the bases of all records without gaps + a record table (csrc/fasta_kernels.hip),
 *                      with the semantics of megapath_nano_amd/fastx.py iter_fastx.
 *
 * and of BAM files as read input (the BGZF blocks of the file are the streams of mpn_gzip_inflate_device; csrc/bam_in_kernels.hip):
 *
 *   mpn_bam_flatten    the inflated slots of a group of blocks -> one contiguous BAM text, behind the unconsumed tail of the group before
 *                      (a chunked gather: its search, 16-byte load and launch shape are csrc/gather16.h, shared with mpn_reads.h)
 *   mpn_bam_walk       the text -> a table with a row per record (the walk itself is csrc/bam_walk_core.h, which also compiles
 *                      for the host)
 *   mpn_bam_decode     the rows of a batch of reads -> ASCII bases, Phred+33 qualities and names, reads that are stored as their
 *                      reverse complement restored, in the layout of mapper.PackedReads.from_arrays
 *
 * and of FASTQ files as read input (MPN_READ_INGEST=device; csrc/fastq_scan_kernels.hip -- csrc/fastq_kernels.hip is the quality
 * filter of mpn_fastq.h).  The text comes from the file as it is, from zlib on the host, or from mpn_gzip_inflate_device and
 * mpn_bam_flatten when the file is BGZF:
 *
 *   mpn_fastq_scan     the text -> a table with a row per plain four-line record, for the longest prefix of such records
 *   mpn_fastq_gather   the rows of a batch of reads -> bases, qualities and names in the layout of mpn_bam_decode (gather16.h)
 *
 * and of the read filter on such a text (csrc/fastq_filter_kernels.hip; the arithmetic is defined in mpn_fastq.h):
 *
 *   mpn_fastq_heads      the rows -> the headers as the host filter reads them: id, separator, comment
 *   mpn_fastq_qsum_rows  the rows -> the error sums of mpn_fastq_qsum_batch from the qualities where they lie
 *   mpn_fastq_emit       chosen rows, cropped -> their FASTQ text (gather16.h)
 *
 * and of the name lists that `nanosplit` and `seqtk subseq` (fastx.py) match the records of such a text against
 * (csrc/name_lookup_kernels.hip; the table is csrc/name_set_core.h, which also compiles for the host):
 *
 *   mpn_name_set_create    a list of names -> a hash table of them in HBM, built on the host
 *   mpn_fastq_name_lookup  the headers -> the list entry each record's id is, the ids staying on the device
 *
 * Grouping of files, slot sizing, the fallbacks to the host path and the cutting into index parts are in
 * megapath_nano_amd/ingest.py.  Calling rules as for mpn_bgzf_compress: a call returns when its results are on the host, the
 * default stream is used, -1 = device error (mpn_last_error()), -2 = bad arguments.
 */
#ifndef MPN_INGEST_H
#define MPN_INGEST_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* What became of one stream.  Anything but OK and OVERFLOW: the bytes of the slot are not to be used. */
enum {
    MPN_INFLATE_OK = 0,
    MPN_INFLATE_TRUNCATED = 1,    /* the input ends inside a member */
    MPN_INFLATE_BAD_MAGIC = 2,    /* bytes that are neither a gzip member (1f 8b, CM = 8) nor zero padding after one */
    MPN_INFLATE_BAD_BLOCK = 3,    /* block type 3, or LEN / NLEN of a stored block disagree */
    MPN_INFLATE_BAD_CODE = 4,     /* over-subscribed or wrongly incomplete code, a bit pattern or symbol without meaning */
    MPN_INFLATE_BAD_DISTANCE = 5, /* a distance further back than the member's output */
    MPN_INFLATE_BAD_CRC = 6,
    MPN_INFLATE_BAD_SIZE = 7,     /* ISIZE is not the member's length mod 2^32 */
    MPN_INFLATE_OVERFLOW = 8,     /* well-formed, but longer than its slot: out_len is exact, the slot holds its first bytes */
    MPN_FASTA_UNSUPPORTED = 9,    /* mpn_fasta_scan only: text iter_fastx would not read as plain FASTA records */
    MPN_BAM_TRUNCATED = 10,       /* mpn_bam_walk only, as are the next three: the header or a record passes the end of the last text */
    MPN_BAM_BAD_MAGIC = 11,       /* the text does not start with BAM\1 */
    MPN_BAM_BAD_HEADER = 12,      /* a negative l_text or n_ref, a reference name of less than one byte */
    MPN_BAM_BAD_RECORD = 13,      /* block_size < 32, l_read_name < 1, l_seq < 0, or name, CIGAR, bases and qualities longer than block_size */
    MPN_FASTQ_UNSUPPORTED = 14    /* mpn_fastq_scan only: the record at *consumed is not a plain four-line record (or, with final, is cut short) */
};

/* n streams: stream i is in[in_off[i] .. in_off[i + 1]), a whole file: zero or more gzip members back to back, zero bytes
 * after the last one allowed.  Its bytes go to out[slot_off[i] .. slot_off[i] + min(out_len[i], slot_cap[i])); nothing else of out
 * is written.  slot_off[i] must be a multiple of 16 and the slots must not overlap.  out_len[i]: the inflated length (exact for
 * OK and OVERFLOW), n_members[i]: the members that were complete and verified (CRC-32 and ISIZE of each), status[i]: MPN_INFLATE_*.
 * Malformed input ends in a status, never in an access outside the stream or the slot.  All pointers are HOST pointers (out is
 * uploaded and downloaded whole: the call exists for tests).  Returns 0. */
int32_t mpn_gzip_inflate(int64_t n, const uint8_t *in, const int64_t *in_off /* n + 1 */, uint8_t *out, const int64_t *slot_off,
                         const int64_t *slot_cap, int64_t *out_len, int32_t *n_members, int32_t *status);

/* The same with the compressed bytes and the slots in HBM: d_in (in_off[0] is its first byte's offset: d_in[in_off[i] - in_off[0]])
 * and d_out are DEVICE pointers, d_out 16-byte aligned; the other arrays are host arrays. */
int32_t mpn_gzip_inflate_device(int64_t n, const void *d_in, const int64_t *in_off /* n + 1 */, void *d_out, const int64_t *slot_off,
                                const int64_t *slot_cap, int64_t *out_len, int32_t *n_members, int32_t *status);

/* FASTA text of n streams in HBM: stream i is d_text[text_off[i] .. text_off[i] + text_len[i]) (DEVICE pointer; host arrays).
 * A record starts at a line whose first byte is '>' (line starts reset at every stream start); its name is the first word of
 * that line; CR and LF vanish; everything else of the other lines is sequence, unchanged.
 *
 * Counting call (d_seq = NULL, rec_cap = 0): n_records / n_bases [i] and status[i] (MPN_INFLATE_OK or MPN_FASTA_UNSUPPORTED) of
 * every stream.  UNSUPPORTED: sequence bytes before the first header, a line that starts with '@' or '+', a blank, tab, VT or FF
 * in a sequence line, or a CR that is not part of a line end.
 * Full call: additionally the bases of all records of all streams, without gaps in stream and record order, at d_seq (DEVICE
 * pointer, seq_cap bytes); rec_stream / rec_name_off (into d_text) / rec_name_len / rec_seq_len [r] for r < sum of n_records;
 * and the names one after another in name_pool (name_pool_cap bytes, host).  Returns 0, or -3 if a capacity is too small
 * (n_records / n_bases are complete, nothing else is). */
int32_t mpn_fasta_scan(int64_t n, const void *d_text, const int64_t *text_off, const int64_t *text_len, void *d_seq, int64_t seq_cap,
                       int64_t *n_records, int64_t *n_bases, int32_t *status, int64_t rec_cap, int32_t *rec_stream,
                       int64_t *rec_name_off, int32_t *rec_name_len, int64_t *rec_seq_len, char *name_pool, int64_t name_pool_cap);

/* Device time of the calling thread's last mpn_gzip_inflate[_device] and last mpn_fasta_scan by HIP events, in milliseconds.
 * Either pointer may be NULL. */
void mpn_ingest_last_device_ms(double *inflate_ms, double *scan_ms);

/* ---- BAM as read input ---------------------------------------------------------------------------------------------------------
 * A row of the record table: where the record starts in the text (at its block_size field) and what its 32 fixed bytes say. */
typedef struct {
    int64_t off;
    int32_t l_seq;
    uint16_t flag;
    uint8_t l_read_name;     /* with the NUL */
    uint8_t has_qual;        /* 1: l_seq > 0 and the first quality byte is not 0xFF */
} mpn_bam_row;

/* n pieces of inflated text, piece i at d_slots[slot_off[i] .. + slot_len[i]) (DEVICE pointer; host arrays), are copied one behind
 * the other to d_text (DEVICE, 16-byte aligned), behind the carry_len bytes at d_carry (DEVICE; any alignment, must not overlap
 * d_text): d_text[0 .. carry_len + sum of slot_len), and zeros up to the next multiple of 16, which text_cap must hold.  *text_len:
 * the bytes of text.  A wave per MPN_BAM_CHUNK bytes of output. */
#define MPN_BAM_CHUNK 1024
int32_t mpn_bam_flatten(int64_t n, const void *d_slots, const int64_t *slot_off, const int64_t *slot_len, const void *d_carry,
                        int64_t carry_len, void *d_text, int64_t text_cap, int64_t *text_len);

/* Walks d_text[start .. text_len) (DEVICE pointer): with at_header the BAM header first (magic, l_text, n_ref, the reference
 * entries), then at most max_records records along their block_size fields.  rows[0 .. *n_records) (host, max_records entries) are
 * the records that were whole and well-formed, *next is the offset of the first byte that was not consumed and *status is
 *   MPN_INFLATE_OK       the walk reached the end of the text, max_records, or -- without final -- a header or record that passes
 *                        the end of the text: *next is its start, and the caller carries text[*next ..) to the front of the next
 *                        text.  With at_header, *next > start exactly when the header was whole.
 *   MPN_BAM_TRUNCATED    with final: a header or record passes the end of the text
 *   MPN_BAM_BAD_MAGIC, MPN_BAM_BAD_HEADER, MPN_BAM_BAD_RECORD    (*next: the offending header or record)
 * Malformed input ends in a status and never in an access outside the text.  One wave: lane 0 follows the chain, the lanes read the
 * fixed fields of 64 records at a time.  Returns 0. */
int32_t mpn_bam_walk(const void *d_text, int64_t text_len, int64_t start, int32_t at_header, int32_t final, int64_t max_records,
                     mpn_bam_row *rows, int64_t *n_records, int64_t *next, int32_t *status);

/* The reads of n rows (host; of mpn_bam_walk on this d_text, the caller has dropped the records it skips): read r's bases go to
 * d_seq[out_off[r] .. + l_seq) (DEVICE; out_off: host, the exclusive sum of l_seq) as ASCII through =ACMGRSVTWYHKDBN, a record with
 * flag 0x10 reversed and complemented; with d_qual (DEVICE, or NULL) its qualities + 33 to the same place of d_qual, reversed
 * alike, '!' for a row without has_qual.  Both buffers are 16-byte aligned and hold total = out_off[n - 1] + l_seq[n - 1] bytes, + 16,
 * rounded up to a multiple of 16: what follows the last base is zeroed.  The names (l_read_name - 1 bytes each) go one behind the
 * other to name_pool (host, name_pool_cap bytes).  Returns 0, -2 for arguments or rows that do not fit the text (nothing outside it
 * is read), -3 if name_pool_cap is too small. */
int32_t mpn_bam_decode(const void *d_text, int64_t text_len, int64_t n, const mpn_bam_row *rows, const int64_t *out_off, void *d_seq,
                       void *d_qual, char *name_pool, int64_t name_pool_cap);

/* Device time of the calling thread's last mpn_bam_flatten, mpn_bam_walk and mpn_bam_decode, as mpn_ingest_last_device_ms gives it
 * for the first two stages.  Any pointer may be NULL. */
void mpn_bam_last_device_ms(double *flatten_ms, double *walk_ms, double *decode_ms);

/* ---- FASTQ as read input -------------------------------------------------------------------------------------------------------
 * A row of the record table: where the bases, the qualities (len bytes each) and the name (name_len bytes) lie in the text. */
typedef struct {
    int64_t seq_off, qual_off, name_off;
    int32_t len, name_len;
} mpn_fastq_row;

/* The scan works on tiles of this many bytes (lines may be of any length; the tests place their edge cases by it). */
#define MPN_FASTQ_TILE 4096
int32_t mpn_fastq_tile(void);

/* d_text[0 .. text_len) (DEVICE pointer) starts at a record start.  The kind of a line is its index modulo 4, counted in line feeds
 * from the start of the text.  A record is PLAIN when
 *   line 0  starts with '@' (the name is the first word behind it, with the separators of Python's bytes.split());
 *   line 1  starts with none of '@', '>', '+' and holds no blank, TAB, VT or FF (it may be empty);
 *   line 2  starts with '+' (the rest of it is ignored);
 *   line 3  has exactly as many bytes as line 1 (it may start with '@', '+' or '>');
 *   a CR in lines 0, 1 and 3 stands directly before the LF (and is dropped with it);
 *   the read is no longer than 2^31 - 1 bases.
 * The scan takes the longest prefix of plain records: rows[0 .. *n_records) (host, rec_cap entries), *consumed = the offset behind
 * the last line end of that prefix, and *status is
 *   MPN_INFLATE_OK          the text ended at *consumed -- or, without final, inside the record that starts at *consumed: the caller
 *                           carries text[*consumed ..) to the front of the next text.  With final, a last line without LF is whole.
 *   MPN_FASTQ_UNSUPPORTED   the record at *consumed is not plain; with final also: it is cut short.  fastx.iter_fastx continues there.
 * Counting call (rows = NULL, rec_cap = 0): n_records, consumed and status only.  Returns 0, or -3 if rec_cap is too small
 * (*n_records, *consumed and *status are complete, rows is not).  Malformed input ends in a status and never in an access outside
 * the text.  Device memory: 8 bytes per line and 32 per record next to the text. */
int32_t mpn_fastq_scan(const void *d_text, int64_t text_len, int32_t final, int64_t rec_cap, mpn_fastq_row *rows, int64_t *n_records,
                       int64_t *consumed, int32_t *status);

/* The reads of n rows (host; of mpn_fastq_scan on this d_text, any subset in any order): read r's bases go to
 * d_seq[out_off[r] .. + len) (DEVICE; out_off: host, the exclusive sum of len) and, with d_qual (DEVICE, or NULL), its qualities to the
 * same place of d_qual, both unchanged.  Layout and return codes as mpn_bam_decode: both buffers are 16-byte aligned and hold
 * total + 16 bytes rounded up to a multiple of 16, what follows the last base is zeroed, the names go one behind the other to
 * name_pool (host); -2 for arguments or rows that do not lie inside the text (nothing outside it is read), -3 if name_pool_cap is
 * too small. */
int32_t mpn_fastq_gather(const void *d_text, int64_t text_len, int64_t n, const mpn_fastq_row *rows, const int64_t *out_off, void *d_seq,
                         void *d_qual, char *name_pool, int64_t name_pool_cap);

/* Device time of the calling thread's last mpn_fastq_scan and mpn_fastq_gather in milliseconds.  Either pointer may be NULL. */
void mpn_fastq_last_device_ms(double *scan_ms, double *gather_ms);

/* ---- The read filter on the resident text (csrc/fastq_filter_kernels.hip) -------------------------------------------------------
 * What `nanofastq` (megapath_nano_amd/fastq_filter.py; its arithmetic is mpn_fastq.h) and `seqtk subseq` (fastx.subseq) need of a
 * scanned text: the headers with their comments, the error sums of the qualities where they lie, and the FASTQ text of chosen
 * records, cropped.  All four calls take d_text[0 .. text_len) (DEVICE pointer) and host rows of mpn_fastq_scan on that text (any
 * subset in any order, or rows moved inside their lines), read nothing outside the text, and return 0, -1 (device error), -2 (bad
 * arguments, rows that do not lie inside the text: nothing is launched) or -3 (a capacity is too small).
 *
 * The header of a record as the HOST FILTER reads it (fastq_filter.parse_fastx -- not the first-word rule of mpn_fastq_scan): the bytes
 * behind the '@' that opens the line in front of the bases, up to the line end, without the CR of a CRLF.  The line start is found in
 * the text itself, going back from seq_off - 1 to the previous line feed or to offset 0.  The id ends before the first blank or TAB
 * (VT and FF stay inside it; it may be empty); the comment is what follows that one byte. */
typedef struct {
    int64_t off;          /* the offset behind the '@' */
    int32_t id_len;
    int32_t comment_len;  /* bytes behind the separator (from off + id_len + 1); -1: the header has no separator */
} mpn_fastq_head;

/* heads[r] for r < n.  With name_pool (host, name_pool_cap bytes; or NULL and 0) the ids go one behind the other to it, as the names
 * of mpn_fastq_gather do; -3 if it is too small (heads is complete then).  Every row needs seq_off >= 2: a header line in front. */
int32_t mpn_fastq_heads(const void *d_text, int64_t text_len, int64_t n, const mpn_fastq_row *rows, mpn_fastq_head *heads, char *name_pool,
                        int64_t name_pool_cap);

/* total / cropped / status [r] of the qualities text[qual_off .. + len) of row r, with the contract of mpn_fastq_qsum_batch (mpn_fastq.h):
 * sequential IEEE-754 additions in read order, then the head and the tail subtractions one by one, bit-identical doubles; table[128]
 * (host) as there.  One lane per read, 16-byte loads at any alignment of the line.  order (host, n entries, or NULL for 0, 1, ..):
 * a permutation of 0 .. n - 1; lane i of the launch takes row order[i], so that the caller can put reads of similar length into one
 * wave (a wave runs as long as its longest read).  Results are stored by row index.  fastq_filter.py passes NULL: ordering by
 * length did not pay where it was measured (profiles/r18_read_filter/README.md). */
int32_t mpn_fastq_qsum_rows(const void *d_text, int64_t text_len, int64_t n, const mpn_fastq_row *rows, const int32_t *order, int32_t head_crop,
                            int32_t tail_crop, int32_t min_len, const double *table, double *total, double *cropped, uint8_t *status);

/* What is written of record r: bases and qualities [start, start + m) of its row, its comment or not, its own id or a serial. */
typedef struct {
    int32_t start, m;        /* 0 <= start, 0 <= m, start + m <= len */
    int32_t with_comment;    /* 1: ' ' + comment behind the id (comment_len < 0 counts as an empty comment: the blank alone) */
    int32_t reserved;        /* 0 */
    int64_t serial;          /* 0: the id of the header; > 0: the id is prefix + the decimal digits of serial */
} mpn_fastq_pick;

/* The FASTQ text of n records to d_out (DEVICE, 16-byte aligned): record r is
 *   '@' id [' ' comment] LF  seq[start .. start + m)  LF '+' LF  qual[start .. start + m)  LF
 * at d_out[out_off[r] .. out_off[r + 1]).  out_off (host, n + 1 entries) starts at 0 and is the exclusive sum of these sizes: the call
 * checks that, and that out_cap holds out_off[n] rounded up to a multiple of 16 (what follows the last record up to there is
 * zeroed), before anything is launched (-2 otherwise).  prefix: prefix_len bytes (host) in front of every serial.  Shaped like the other
 * gathers (csrc/gather16.h): a wave per MPN_BAM_CHUNK bytes of output, every byte written once by aligned 16-byte stores. */
int32_t mpn_fastq_emit(const void *d_text, int64_t text_len, int64_t n, const mpn_fastq_row *rows, const mpn_fastq_head *heads,
                       const mpn_fastq_pick *picks, const char *prefix, int32_t prefix_len, const int64_t *out_off, void *d_out, int64_t out_cap);

/* Device time of the calling thread's last mpn_fastq_heads, mpn_fastq_qsum_rows and mpn_fastq_emit.  Any pointer may be NULL. */
void mpn_fastq_filter_last_device_ms(double *heads_ms, double *sums_ms, double *emit_ms);

/* ---- Read names matched on the resident text (csrc/name_lookup_kernels.hip; hash, probe step and slot layout: csrc/name_set_core.h) --
 * A list of n names in HBM as an open-addressing table with linear probing.  Name i is pool[off[i] .. off[i + 1]) (host; any bytes,
 * none included; n may be 0).  The table is built on the host, serially, so its layout depends on the list and on `slots` alone;
 * equal names share one slot, which holds the SMALLEST of their indices, and first_of[i] (host, n entries, or NULL) is that index
 * for every i.  slots = 0: the smallest power of two >= 2 x (distinct names), at least 16; any other value must be a power of two
 * larger than the number of distinct names (-2 otherwise; a small table is how tests force long probe chains).  *set owns device
 * memory until mpn_name_set_free (NULL is allowed there).  Returns 0, -1 (device error, out of memory) or -2. */
typedef struct mpn_name_set mpn_name_set;
int32_t mpn_name_set_create(int64_t n, const char *pool, const int64_t *off /* n + 1 */, int64_t slots, mpn_name_set **set,
                            int32_t *first_of /* n, or NULL */);
void mpn_name_set_free(mpn_name_set *set);

/* found[r] (host, n entries) for the record whose header is heads[r] (host; of mpn_fastq_heads on this d_text): the smallest list index
 * whose bytes are the id d_text[heads[r].off .. + id_len), or -1.  One lane per record; the id and the pooled name are compared by
 * 16-byte loads at any alignment, and a slot whose hash or length differs costs no load from the pool.  Every 16-byte vector that
 * is read from the text holds a byte of an id.  Returns 0, -1, or -2 before anything is launched: a NULL set, a negative id_len, an
 * id that does not lie inside the text. */
int32_t mpn_fastq_name_lookup(const void *d_text, int64_t text_len, int64_t n, const mpn_fastq_head *heads, const mpn_name_set *set,
                              int32_t *found /* n */);

/* Device time of the calling thread's last mpn_fastq_name_lookup.  The pointer may be NULL. */
void mpn_fastq_lookup_last_device_ms(double *lookup_ms);

#ifdef __cplusplus
}
#endif
#endif
