/*
 * mpn_map.h -- C-ABI of the MI355X-native long-read mapper (libmpn.so): the seed-chain-extend path that
 * MegaPath-Nano runs as an external `minimap2` process.
 *
 * Reference interface replaced:  /root/reference/bin/lib/aligner.py:187-231  builds
 *     [aligner, -c, (-a), -t N, -I xG, (-N 50 -p 1), -x map-ont, <target fasta>, <query fastq>...]
 * and reads PAF (or SAM) from the child's stdout (:204-206, :225-231); options come from
 * /root/reference/bin/megapath_nano.py:1124 (human/decoy filter) and :1270 (species placement).
 * The reference has no in-process FFI for this step (it is a process boundary), so the entry points below are
 * what a binding for it needs: build/load an index from target sequences, map a batch of reads, get PAF text
 * with minimap2's `-c` tag order (NM at column 13, AS at column 15, which the awk at aligner.py:271-273
 * relies on).  The Python mirror megapath_nano_amd/aligner.py Align() wraps them behind the reference's own
 * function signature; bin/mpn-aligner is the `--aligner` executable drop-in.
 *
 * Semantics: minimap2 2.17 `-x map-ont` as restated in oracle/mm2_oracle.c (PARITY UNPINNED: minimap2 is not
 * vendored by the reference; DESIGN.md section 6 lists the deliberate differences).
 *
 * Stage entry points (mpn_sketch_batch, mpn_seed_chain_batch, mpn_seed_anchors_batch, mpn_chain_batch, mpn_hit_select_batch,
 * mpn_ext_plan_batch, mpn_ext_dp_batch, mpn_stitch_batch, mpn_aln_finish_batch, mpn_aln_tags_batch) exist so that the parity tests can
 * compare every GPU stage with the oracle or a restatement of it; mpn_map_batch is the product call.
 *
 * Difference strings (minimap2 --cs, --cs=long, --MD, --eqx): mpn_map_opt.out_tags.  The strings are made on the GPU when the
 * alignment is finished, because only there are the read, the fixed CIGAR and the packed target together; they are written
 * for hits that have a CIGAR, in PAF after cg:Z and in SAM before rl:i.  A column of an M op matches iff the two 0..4 codes
 * are equal (N against N matches, unlike in NM).  cs and MD are both written when both are asked for, and MD always ends in
 * a count.
 */
#ifndef MPN_MAP_H
#define MPN_MAP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpn_index mpn_index;

typedef struct {
    /* indexing */
    int32_t k, w;                 /* -k 15 -w 10 (map-ont) */
    /* seeding / chaining */
    float mid_occ_frac;           /* -f 2e-4 */
    int32_t mid_occ;              /* > 0 overrides the quantile */
    int32_t max_gap, bw, max_chain_skip, max_chain_iter, min_cnt, min_chain_score;
    /* hit selection */
    float mask_level, pri_ratio;  /* -p */
    int32_t best_n;               /* -N */
    int32_t max_join_long, max_join_short, min_join_flank_sc;
    float min_join_flank_ratio;
    /* base-level extension (-c) */
    int32_t a, b, q, e, q2, e2, sc_ambi, zdrop, zdrop_inv, end_bonus, min_dp_max, min_ksw_len;
    float max_clip_ratio;
    int64_t max_sw_mat;
    int32_t with_cigar;           /* -c; 0 = mapping_only (aligner.py:188) */
    uint32_t seed;
    int32_t host_threads;         /* threads for the host-side hit bookkeeping; 0 = all cores */
    int32_t out_sam;              /* -a: 1 = the text buffer of mpn_map_batch(_ex) receives SAM records instead of PAF lines
                                   * (aligner.py:188-192; header lines: mpn_sam_header), 2 = PAF lines AND kept SAM records
                                   * (mpn_map_batch_q).  Unmapped reads get a flag-4 record; QUAL is '*' unless the
                                   * qualities are handed over (mpn_map_batch_q, mpn_hits_finish). */
    int32_t out_tags;             /* MPN_TAG_* bits: cs:Z / MD:Z tags and =/X CIGARs on every hit that has a CIGAR (text output with
                                   * with_cigar only; calls that return columns alone ignore it).  0 = none. */
} mpn_map_opt;

enum {
    MPN_TAG_CS = 1,       /* --cs, --cs=short: cs:Z in the short form (:k for k matching columns) */
    MPN_TAG_CS_LONG = 2,  /* --cs=long: cs:Z with the matching bases spelled out (=ACGT); implies MPN_TAG_CS */
    MPN_TAG_MD = 4,       /* --MD */
    MPN_TAG_EQX = 8       /* --eqx: M ops of cg:Z, the SAM CIGAR column and BAM records split into = (op 7) and X (op 8) */
};

/* minimap2 2.17 defaults for `-x map-ont -c` (-N 5 -p 0.8) */
void mpn_map_opt_init(mpn_map_opt *opt);

/* Build the index of n_seq target sequences (ASCII, any case; non-ACGT = ambiguous) and keep it resident in
 * HBM together with the 2-bit packed targets.  Returns NULL on failure (mpn_last_error()). */
mpn_index *mpn_index_build(int32_t n_seq, const char *const *names, const char *const *seqs, const int32_t *lens,
                           int32_t k, int32_t w);
/* The same build from targets that are already resident in HBM: d_seqs is a DEVICE pointer to the concatenated ASCII
 * targets (target i at byte seq_off[i], seq_off[0] = 0, no gaps; seq_off and lens are host arrays).  The caller keeps
 * ownership of d_seqs and may release it when the call returns.  This is how a target set that never exists as host
 * strings (a decompressor or generator writing into HBM; bench.py's synthetic RefSeq stand-in) is indexed. */
mpn_index *mpn_index_build_device(int32_t n_seq, const char *const *names, const void *d_seqs, const int64_t *seq_off,
                                  const int32_t *lens, int32_t k, int32_t w);
void mpn_index_destroy(mpn_index *idx);
/* Persistent form of a built index (the reference rebuilds its index on every run: bin/lib/aligner.py:209-221; minimap2's
 * own `-d FILE` / prebuilt-index-as-target is used at bin/megapath_nano.py:1641-1645).  save: 0 or negative error;
 * load: a resident index equal to the one saved (same keys/positions/targets), or NULL + mpn_last_error(). */
int mpn_index_save(const mpn_index *idx, const char *path);
/* "@SQ" lines of the targets + one "@PG" line (cmdline may be NULL); returns the text length, or -3 if cap is too small */
int64_t mpn_sam_header(const mpn_index *idx, const char *cmdline, char *buf, int64_t cap);
mpn_index *mpn_index_load(const char *path);
/* A target set of several index parts (minimap2 -I) in ONE file, as minimap2 -d dumps it (bin/megapath_nano.py:1641-1645):
 * save_append adds a part behind what the file holds; load_at reads the part that starts at byte `offset` and leaves in
 * *next_offset where the next one starts, or -1 after the last (next_offset may be NULL). */
int mpn_index_save_append(const mpn_index *idx, const char *path);
mpn_index *mpn_index_load_at(const char *path, int64_t offset, int64_t *next_offset);
/* The part at `offset` without loading it: returns its number of targets (*bases: their total length; *next_offset as above), or -1 */
int32_t mpn_index_part_info(const char *path, int64_t offset, int64_t *bases, int64_t *next_offset);
/* names and lengths of the targets of an index (for a loaded one): name i is copied into buf (cap bytes incl. NUL) */
int32_t mpn_index_n_seq(const mpn_index *idx);
int32_t mpn_index_seq_len(const mpn_index *idx, int32_t i);
int32_t mpn_index_seq_name(const mpn_index *idx, int32_t i, char *buf, int32_t cap);
int32_t mpn_index_k(const mpn_index *idx);
int32_t mpn_index_w(const mpn_index *idx);
int64_t mpn_index_n_minimizers(const mpn_index *idx);
int64_t mpn_index_n_keys(const mpn_index *idx);
/* occurrence cut-off for a given -f (minimap2: mm_idx_cal_max_occ) */
int32_t mpn_index_mid_occ(const mpn_index *idx, float frac);
/* bases [start, start+len) of target i as upper-case ASCII (ambiguous bases come back as 'N'), decoded from the 2-bit
 * targets resident in HBM: what a checker of PAF lines needs when the target set is too large to keep on the host
 * (bench.py's correctness block).  Returns len, or a negative error (range outside the target). */
int64_t mpn_index_fetch_seq(const mpn_index *idx, int32_t i, int64_t start, int64_t len, char *out);
/* copies of index arrays for the parity tests: keys[n_keys], key_off[n_keys+1], pos[n_minimizers] */
int mpn_index_export(const mpn_index *idx, uint64_t *keys, int64_t *key_off, uint64_t *pos);

/* ---- stage: (w,k)-minimizers of a batch of sequences, one CSR row per sequence ---------------------------
 * seqs: concatenated ASCII; sequence i = seqs[seq_off[i] .. +seq_len[i]).  mz_off must hold n+1 entries.
 * Minimizers are returned as (x = hash<<8|span, y = i<<32|last_pos<<1|strand) pairs in mz (cap pairs).
 * Returns the total number of minimizers, or a negative error (-3: cap too small; mz_off is still filled). */
int64_t mpn_sketch_batch(int32_t n, const char *seqs, const int64_t *seq_off, const int32_t *seq_len, int32_t k,
                         int32_t w, int64_t *mz_off, uint64_t *mz, int64_t cap);

/* ---- stage: seeds -> sorted anchors -> chains, for a batch of reads --------------------------------------
 * Outputs (caller allocated; CSR over reads):
 *   n_anchor[i], rep_len[i]               anchors found / repetitive-minimizer span (minimap2 rl:i)
 *   chain_off[n+1], chains u[] (score<<32|cnt), achor_off[n+1], chained anchors b[] as (x, y) pairs
 * Returns 0, or negative error (-3: a capacity is too small; -1 also for opt->max_gap above 66076418, the largest for which the
 * chain DP's 32-bit running coordinate cannot wrap: every mapping call refuses it the same way). */
int mpn_seed_chain_batch(const mpn_index *idx, const mpn_map_opt *opt, int32_t n, const char *seqs,
                         const int64_t *seq_off, const int32_t *seq_len, int64_t *n_anchor, int32_t *rep_len,
                         int64_t *chain_off, uint64_t *u, int64_t u_cap, int64_t *anchor_off, uint64_t *b,
                         int64_t b_cap);

/* ---- stage: chaining on arbitrary sorted anchors (tests) --------------------------------------------------------------------------
 * The second half of mpn_seed_chain_batch (minimap2's mm_chain_dp): the drop of segments too short to chain, the cut into work items,
 * the chain DP, the chain ends, their sort and the backtrack with the chain records, run by the same function with the same launches
 * as the mapper's.  Read i has the anchors anchors[anchor_off[i] .. anchor_off[i + 1]) as (x, y) word pairs (x = strand << 63 |
 * rid << 32 | target position, y = flags << 40 | span << 32 | read position), sorted as the anchor sort leaves them (ascending x,
 * then y).  The gap cost's average seed length of a read is taken over ALL the anchors given for it, also those in segments the
 * compaction drops.  Of opt only max_gap, bw, max_chain_skip, max_chain_iter, min_cnt and min_chain_score are read.
 * chain_item: 0 = the mapper's value (or MPN_CHAIN_ITEM), else the anchors from which a run of segments is a work item (held to
 * 16 .. 4096); bt_par_min: 0 = the mapper's value (or MPN_BT_PAR_MIN), else the number of chain ends from which the backtrack runs a
 * lane per end; grid_cap: 0 = the mapper's grids, else at most that many blocks for every launch that walks its reads, pieces or
 * queue with a stride (the per-read table kernel and the scans have a thread per element and are not capped).
 * Validated on the host before any launch (-1): offsets that start at 0 and do not decrease; within a read x never decreasing;
 * every read position (the low 32 bits of y) in 0 .. 2^31 - 1; no negative option; max_chain_iter >= 1; max_gap <= 66076418 (see
 * mpn_seed_chain_batch); chain_item, bt_par_min, grid_cap >= 0.
 * Out: n_chain[n], n_chained[n]; per read in the order of mpn_seed_chain_batch (chains by their first anchor), read after read:
 * u (score << 32 | cnt) and recs, 6 words per chain: fx, fy, lx, ly (first and last anchor, bit for bit), mlen, blen
 * (mm_cal_fuzzy_len), room for u_cap chains each; b: the chained anchors as (x, y) pairs, chain after chain, room for b_cap.
 * Returns 0, -3 if a capacity is too small (n_chain and n_chained are filled), or -1. */
int mpn_chain_batch(const mpn_map_opt *opt, int32_t n, const int64_t *anchor_off, const uint64_t *anchors, int32_t chain_item,
                    int32_t bt_par_min, int32_t grid_cap, int32_t *n_chain, int64_t *n_chained, uint64_t *u, int64_t *recs,
                    int64_t u_cap, uint64_t *b, int64_t b_cap);

/* ---- stage: hit lookup, stray-hit filter, anchor emission and anchor sort on a made index and made minimizers (tests) -----------
 * The first half of mpn_seed_chain_batch (minimap2's mm_collect_matches and the sort behind it), run by the same function with the
 * same launches, grids and scratch as the mapper's.
 * The index: k, n_seq targets of lens[] bases, keys[n_keys] strictly ascending below 2^(2k), key_off[n_keys + 1], pos[key_off[n_keys]]
 * in the index's own layout (rid << 32 | position << 1 | strand, ascending inside a key).  The entry builds a temporary index from
 * them the way the loader does (the bucket table and the (key, offset) pairs are the mapper's own); no target bases are needed.
 * The minimizers: read i has mz[mz_off[i] .. mz_off[i + 1]) as (x, y) word pairs in the sketch's layout (x = hash << 8 | span,
 * y = read << 32 | last_pos << 1 | strand) and seq_len[i] bases.  Nothing is sketched.
 * Of opt only mid_occ (explicit, 1 .. 2^25), min_cnt and max_gap are read.  flt_round2: 0 = the mapper's value (MPN_FLT_ROUND2, off),
 * else the hits from which a read is counted twice by the filter; flt_wgs: 0 = the mapper's value (MPN_FLT_WGS, 256), else the
 * filter's workgroups; grid_cap: 0 = the mapper's grids, else at most that many blocks for every launch that walks its work with a
 * stride or pulls it from a queue (the scans, the order kernel and the per-read offset kernel are not capped).
 * Validated on the host before any launch (-1, the message names the entry): offsets that start at 0 and do not decrease; keys
 * ascending and inside 2k bits; every position inside its target; every minimizer's hash inside 2k bits, span in 1 .. 255 and at
 * most last_pos + 1, last_pos below seq_len and never decreasing inside a read; mid_occ in 1 .. 2^25; no negative option, knob or
 * capacity; max_gap <= 66076418 (see mpn_seed_chain_batch).
 * Out, per read: n_anchor (ALL hits of its minimizers), rep_len, span_sum (the sum of the seed lengths over all hits);
 * anchor_off[n + 1] and the sorted anchors that passed the stray-hit filter as (x, y) pairs, room for cap; counts[0..2]: the buckets
 * the sort put on its three work lists (17..1024, 1025..4096, more anchors), counts[3]: the hits the filter walked (every hit in
 * the first round, a read's survivors in its second).
 * Returns 0, -3 if cap is too small (everything but the anchors is filled), or -1. */
int mpn_seed_anchors_batch(int32_t k, int32_t n_seq, const int32_t *lens, int64_t n_keys, const uint64_t *keys, const int64_t *key_off,
                           const uint64_t *pos, const mpn_map_opt *opt, int32_t n, const int64_t *mz_off, const uint64_t *mz,
                           const int32_t *seq_len, int64_t flt_round2, int32_t flt_wgs, int32_t grid_cap, int64_t *n_anchor, int32_t *rep_len,
                           int64_t *span_sum, int64_t *anchor_off, uint64_t *anchors, int64_t cap, int64_t counts[4]);

/* ---- stage: the banded dual-affine extension DP on arbitrary pairs of 0..4 code strings (parity tests) -------
 * flag bits as in ksw2: 0x02 approximate max, 0x08 right-align gaps, 0x40 extension only, 0x80 reversed CIGAR.
 * force_kernel: 0 = dispatch as mpn_map_batch does, 1 = LDS-state workgroup kernel with one wave per window, 3 = the same with 256, 512 or 1024 threads by band width, 4 = systolic strip kernel where eligible, 5 = band-in-registers kernel where the band fits 1024 slots, 6 = tiled strips where eligible.  out9[i*9..] = max, zdropped, max_q, max_t, mqe, mqe_t, score, reach_end, n_cigar.
 * Validated on the host before any launch (-1): no array missing, no negative length, offsets from 0 with every pair's end at most
 * 2^30 - 1 (the end of the last pair is taken for the size of qcodes and tcodes).  Returns 0, -3 if cigar_cap is too small, or -1. */
int mpn_ext_dp_batch(const mpn_map_opt *opt, int32_t n, const uint8_t *qcodes, const int64_t *q_off, const int32_t *q_len,
                     const uint8_t *tcodes, const int64_t *t_off, const int32_t *t_len, const int32_t *w, const int32_t *zdrop,
                     const int32_t *end_bonus, const int32_t *flag, int32_t force_kernel, int32_t *out9, uint32_t *cigar_pool,
                     int64_t cigar_cap, int64_t *cig_off);

/* ---- stage: the difference-string kernel on arbitrary alignments (tests) ---------------------------------------------------
 * Pair i: read codes qcodes[q_off[i] .. +q_len[i]) (read orientation), of which [qs[i], qe[i]) is aligned on strand rev[i]
 * (1 = the reverse complement of the interval is what the CIGAR walks); target codes tcodes[t_off[i] .. +t_len[i]) from ts[i];
 * CIGAR cigar[cig_off[i] .. +n_cigar[i]) as len<<4|op with op 0 M, 1 I, 2 D only.  Validated on the host before any launch:
 * no other op, no empty op, exactly qe-qs read bases consumed, inside the target; else -1.  Outputs by out_tags (MPN_TAG_*):
 * cs / md bytes (no NUL) and eqx ops concatenated in pair order, pair i at [*_off[i], *_off[i+1]) (n+1 entries each; outputs
 * that are not asked for may be NULL).  A pair with n_cigar = 0 has no alignment and gets empty outputs.  Returns 0, -3 if a cap
 * is too small, -1 on bad arguments or a device error. */
int mpn_aln_tags_batch(int32_t n, const uint8_t *qcodes, const int64_t *q_off, const int32_t *q_len,
                       const int32_t *qs, const int32_t *qe, const int32_t *rev,
                       const uint8_t *tcodes, const int64_t *t_off, const int32_t *t_len, const int32_t *ts,
                       const uint32_t *cigar, const int64_t *cig_off, const int32_t *n_cigar, int32_t out_tags,
                       char *cs, int64_t cs_cap, int64_t *cs_off, char *md, int64_t md_cap, int64_t *md_off,
                       uint32_t *eqx, int64_t eqx_cap, int64_t *eqx_off);

/* ---- stage: the CIGAR finishing kernel on arbitrary alignments (tests) ------------------------------------------------------
 * What every reported alignment passes through (minimap2's mm_fix_cigar + mm_update_extra), launched exactly as mpn_map_batch
 * launches it.  Pairs as for mpn_aln_tags_batch, but ops of length 0 are allowed; scoring (a, b, sc_ambi, q, e) from opt.
 * Validated on the host before any launch: only ops 0..2, exactly qe-qs read bases consumed, inside the target; else -1.
 * force_class: 0 = the launch class by need as in the product, 1 / 2 / 3 = the 16 / 32 / 64 KB LDS class for every pair (-1 if a
 * pair does not fit), 4 = the global-scratch instantiation for all.  out8[i*8..] = n_cigar, qshift, tshift, blen, mlen,
 * n_ambi, dp_max, 0; the fixed CIGAR of pair i at cigar_out[cig_off[i] .. +n_cigar) (cigar_out as large as cigar).  A pair with
 * n_cigar = 0 is not launched and returns zeros.  Returns 0, or -1 on bad arguments or a device error. */
int mpn_aln_finish_batch(const mpn_map_opt *opt, int32_t n, const uint8_t *qcodes, const int64_t *q_off, const int32_t *q_len,
                         const int32_t *qs, const int32_t *qe, const int32_t *rev,
                         const uint8_t *tcodes, const int64_t *t_off, const int32_t *t_len, const int32_t *ts,
                         const uint32_t *cigar, const int64_t *cig_off, const int32_t *n_cigar, int32_t force_class,
                         int32_t *out8, uint32_t *cigar_out);

/* ---- stage: hits from chains on arbitrary chains (tests) ---------------------------------------------------------------------
 * What mpn_map_batch does between chaining and the alignment rounds (minimap2's mm_gen_regs, mm_set_parent, mm_select_sub,
 * mm_squeeze_a, mm_join_long), run by the same function with the same launches.  Arrays are CSR over reads.  Per chain, in pool
 * order (arbitrary; chain c's anchors follow those of the read's chains before it): u = score << 32 | cnt and the chain record
 * fx, fy, lx, ly, mlen, blen as the backtracking kernel leaves it.  anchors: (x, y) word pairs.  names[i] (may be NULL) is hashed
 * as the mapper hashes it; min_diff = 2k.
 * path: 0 = the mapper's dispatch (small / large kernel instantiation by chain count, host above max_chains), 1 = the large
 * instantiation for every read of at most max_chains chains, 2 = the host functions for every read.  max_chains: 0 = 384, else
 * 1..384.  grid_cap: 0 = the mapper's grids, else at most that many blocks per launch.
 * Validated on the host before any launch (-1): q_len > 0, every cnt >= 1 and the counts add up to the read's anchors, every
 * record equal to its chain's first and last anchor, the x words of the first anchors distinct within a read.
 * Out: n_regs[n], n_a[n]; hits: 15 words per hit, read after read in hit order (room for one per chain): fx, fy, lx, ly, score,
 * score0, cnt, as, parent, subsc, n_sub, mlen, blen, hash, sam_pri; with opt->with_cigar sq_anchors: the squeezed anchor lists,
 * read after read, as (x, y) pairs (room for every anchor), else untouched.  Returns 0, or -1. */
int mpn_hit_select_batch(const mpn_map_opt *opt, int32_t k, int32_t n, const int32_t *q_len, const char *const *names,
                         const int64_t *chain_off, const uint64_t *u, const uint64_t *fx, const uint64_t *fy, const uint64_t *lx,
                         const uint64_t *ly, const int32_t *mlen, const int32_t *blen, const int64_t *anchor_off, const uint64_t *anchors,
                         int32_t path, int32_t max_chains, int32_t grid_cap, int32_t *n_regs, int32_t *n_a, int64_t *hits,
                         uint64_t *sq_anchors);

/* ---- stage: the planning of the base-level extension on arbitrary hits (tests) ----------------------------------------------------
 * The first half of minimap2's mm_align1 for every hit of an alignment round (mm_fix_bad_ends, mm_filter_bad_seeds, the limits of
 * the two end extensions, the cut of the hit into left extension, gap fills and right extension), run by the same function with
 * the same launch as a round of mpn_map_batch.  t_len: n_targets target lengths.  Arrays are CSR over reads: read i has the
 * squeezed anchors anchors[anchor_off[i] .. anchor_off[i + 1]) as (x, y) word pairs (x = strand << 63 | rid << 32 | target
 * position, y = flags | span << 32 | read position on the hit's strand; the flag bits 40..42 may be set, as a first round leaves
 * them) and the hits hit_off[i] .. hit_off[i + 1): h_as, h_cnt (its anchors [as, as + cnt) of the read's list), h_mlen,
 * h_split_inv.  grid_cap: 0 = the mapper's grid, else at most that many blocks.
 * Validated on the host before any launch (-1): q_len > 0; every anchor with rid < n_targets, 0 <= (int32)x < t_len[rid],
 * 0 <= (int32)y < q_len, span in 1..255 and no bit above 42; every hit with cnt >= 1 and as + cnt within the read's anchors, one
 * x >> 32 for all its anchors, x and y strictly increasing; the hits of a read disjoint; win_cap at least the sum of cnt + 1.
 * Out: hits_out: 11 words per hit in input order: n_jobs, as1, cnt1 (the anchors mm_fix_bad_ends keeps) and qs, rs, qe, re, qs0,
 * qe0, rid, rev of the stitching record; win_out: 13 words per window: read, rid, rev, qs, qlen, ts, tlen, reversed, w, zdrop,
 * end_bonus, flag, job_anchor (the anchor a gap fill ends at, counted from as1; -1 for an extension), the windows of a hit in
 * order (left extension, fills, right extension), hit after hit in input order; *n_win their number; anchors_out: every anchor
 * word as the kernel left it in device memory (SEED_IGNORE marks, bit 41 of y).  A window refused by max_sw_mat is a placeholder
 * with qlen = tlen = w = zdrop = end_bonus = 0 and flag | 0x100.  Returns 0, or -1. */
int mpn_ext_plan_batch(const mpn_map_opt *opt, int32_t k, int32_t n_targets, const int32_t *t_len, int32_t n, const int32_t *q_len,
                       const int64_t *anchor_off, const uint64_t *anchors, const int64_t *hit_off, const int32_t *h_as,
                       const int32_t *h_cnt, const int32_t *h_mlen, const int32_t *h_split_inv, int32_t grid_cap,
                       int32_t *hits_out, int64_t win_cap, int64_t *n_win, int32_t *win_out, uint64_t *anchors_out);

/* ---- stage: the stitching of a hit's DP windows on arbitrary hits, windows and window results (tests) -------------------------------
 * The second half of minimap2's mm_align1 for every hit of an alignment round (the windows' CIGARs appended in order with
 * mm_append_cigar's merge, the DP score, the end coordinates, the cut at the first gap fill that z-dropped or got no DP, the anchor
 * the hit is split at and the measures of its two halves), run by the same function with the same launch as a round of
 * mpn_map_batch.  Read i has the squeezed anchors anchors[anchor_off[i] .. anchor_off[i + 1]) as (x, y) word pairs.
 * hits: 15 words per hit: read, rid, rev, as, cnt (its anchors), as1, cnt1 (those mm_fix_bad_ends kept), qs, rs, qe, re, qs0, qe0
 * (the stitching record), first_win, n_win (its windows wins[first_win .. first_win + n_win): left extension if any, fills in
 * order, right extension if any).  wins: 13 words per window: flag (0x40 extension, 0x100 placeholder without DP, 0x200 inversion
 * found by the z-drop test; 0x02, 0x08, 0x80 are carried), reversed, qs, ts, job_anchor (the anchor a fill ends at, counted from
 * as1; -1 for an extension), and of its result max, zdropped, max_q, max_t, mqe_t, score, reach_end, n_cigar; cig_pos[w]: where its
 * n_cigar operations lie in compact[n_compact].  grid_cap: 0 = the mapper's grid, else at most that many blocks.
 * Validated on the host before any launch (-1): every hit with read < n, rev 0 / 1, cnt >= 1, as + cnt within the read's anchors,
 * as <= as1, cnt1 >= 1, as1 + cnt1 <= as + cnt, coordinates within +-2^28; the hits' window ranges inside wins and disjoint; flags
 * among the six above; an extension (0x40) with job_anchor -1, without 0x200, first if reversed and last if not; a fill not
 * reversed, with job_anchor in 1 .. cnt1 - 1 and not 0x100 and 0x200 at once; of a window without 0x100 (the result of a
 * placeholder is never read): zdropped and reach_end 0 / 1, max and score within +-2^28, max_q, max_t, mqe_t in -1 .. 2^28, its
 * operations inside compact, of kinds 0..2 (M, I, D) and shared with no other window; the operations of a hit shorter than 2^28
 * bases in all (merged lengths are added in place); min_cnt >= 0; pool_cap at least the operations of all windows without 0x100.
 * Out: out: 25 words per hit in input order: the kernel's StitchOut (cig_off, n_ops, dp_score, rs1, re1, qs1, qe1, has_p, dropped,
 * drop_fill, drop_max_t, drop_max_q, split_n, split_inv, split_rec) and FinJob (cig_off, code_off, n_cigar, read, rid, rev, qs1,
 * rs1, qspan, tspan); pool_out: the stitched CIGARs (hit h at cig_off, n_ops words; the order of the hits is the kernel's),
 * *pool_used the final value of its cursor; splits_out: 8 words per cut hit (record split_rec of its hit): x and y of the first
 * anchor of the remainder, x and y of the last anchor before it, mlen and blen of the left half, of the right half; *n_splits
 * their number (room for one per hit).  Returns 0, or -1. */
int mpn_stitch_batch(int32_t n, const int64_t *anchor_off, const uint64_t *anchors, int32_t n_hits, const int32_t *hits, int64_t n_win,
                     const int32_t *wins, const int64_t *cig_pos, int64_t n_compact, const uint32_t *compact, int32_t min_cnt,
                     int32_t grid_cap, int64_t *out, int64_t pool_cap, uint32_t *pool_out, int64_t *pool_used, int64_t *splits_out,
                     int64_t *n_splits);

/* ---- product call: map a batch of reads, PAF text out ----------------------------------------------------
 * names: n NUL-terminated read names.  paf receives the lines of all reads in input order (NUL terminated).
 * Returns the number of bytes written, or negative error (-3: paf_cap too small). */
int64_t mpn_map_batch(const mpn_index *idx, const mpn_map_opt *opt, int32_t n, const char *const *names,
                      const char *seqs, const int64_t *seq_off, const int32_t *seq_len, char *paf, int64_t paf_cap);

/* ---- product call, extended: device-resident reads in, alignment columns out --------------------------------
 * d_seqs/d_off/d_len (DEVICE pointers, may be NULL): the same reads already resident in HBM (bench.py uploads them
 * before the timed region); the host copies are still needed for the CIGAR bookkeeping.
 * paf may be NULL.  cols may be NULL; otherwise every reported alignment fills one row of the caller-allocated
 * arrays (cap rows each), in PAF order: the 12 PAF columns as integers plus NM, AS and the tp flag; these are
 * the fields aligner.py:291-294 keeps.  Returns PAF bytes written (0 if paf is NULL) or a negative error
 * (-3: paf_cap or cols->cap too small; cols->n_rows then holds the required number). */
typedef struct {
    int64_t cap, n_rows;
    int32_t *read_idx, *qs, *qe, *rev, *rid, *rs, *re, *mlen, *blen, *mapq, *nm, *as, *primary;
} mpn_aln_cols;

/* d_seqs (when given): the reads on the device; 4-byte aligned and padded so that the aligned 32-bit word around the
 * last base may be read (any allocation rounded up to 4 bytes will do). */
int64_t mpn_map_batch_ex(const mpn_index *idx, const mpn_map_opt *opt, int32_t n, const char *const *names,
                         const char *seqs, const int64_t *seq_off, const int32_t *seq_len, const void *d_seqs,
                         const int64_t *d_off, const int32_t *d_len, char *paf, int64_t paf_cap, mpn_aln_cols *cols);

/* The general product call: mpn_map_batch_ex plus the reads' base qualities (quals: concatenated like seqs, same offsets, or
 * NULL) for the QUAL column of SAM records.  opt->out_sam: 0 = PAF into paf, 1 = SAM into paf, 2 = PAF into paf AND the SAM
 * records of the same hits kept by the library for mpn_map_fetch_sam (the reference's species-placement call keeps both:
 * bin/lib/aligner.py:183-184,219-227,260-261 -- one mapping pass serves them). */
int64_t mpn_map_batch_q(const mpn_index *idx, const mpn_map_opt *opt, int32_t n, const char *const *names, const char *seqs,
                        const char *quals, const int64_t *seq_off, const int32_t *seq_len, const void *d_seqs, const int64_t *d_off,
                        const int32_t *d_len, char *paf, int64_t paf_cap, mpn_aln_cols *cols);
int64_t mpn_map_fetch_sam(char *buf, int64_t cap);  /* like mpn_map_fetch_text, for the SAM text of out_sam == 2 */

/* ---- split index: minimap2 -I <bases> parts and the --split-prefix merge (bin/lib/aligner.py:199; bin/megapath_nano.py:
 * 4019-4022 passes -I <RAM/64>G, :1124,:1270 pass --split-prefix on every call) ----------------------------------------
 * A target set that exceeds one index is mapped part by part: the caller builds the index of part p, adds the hits of the
 * batch against it (mpn_map_batch_part), destroys it, and after the last part mpn_hits_finish merges per read exactly as
 * minimap2 merges its per-part dumps -- hits pooled with target ids shifted to the concatenated target list,
 * sub-optimal bookkeeping cleared, ranking / parent-secondary grouping / -p -N selection / SAM-primary / MAPQ
 * recomputed over the pool, repetitive-seed length = the largest over the parts -- and emits text and columns like
 * mpn_map_batch_q (column rid and the names in the text refer to the concatenated target list: mpn_hits_seq_*).
 * minimap2 takes the merge path whenever --split-prefix is given, also for a single part. */
typedef struct mpn_hits mpn_hits;
mpn_hits *mpn_hits_create(int32_t n_reads);
void mpn_hits_destroy(mpn_hits *h);
/* want_text = 0: mpn_hits_finish will be asked for the integer columns only (no PAF, no SAM), so the CIGARs of the parts' hits stay in
 * HBM -- the integer fast path of the species-placement step (bin/megapath_nano.py:1262-1299 reads columns only).  Default 1. */
void mpn_hits_set_text(mpn_hits *h, int32_t want_text);
int mpn_map_batch_part(const mpn_index *part, const mpn_map_opt *opt, int32_t n, const char *const *names, const char *seqs,
                       const int64_t *seq_off, const int32_t *seq_len, const void *d_seqs, const int64_t *d_off,
                       const int32_t *d_len, mpn_hits *acc);
/* The same for several parts that are RESIDENT together (an accelerator with room for the whole target set keeps every part in
 * memory instead of streaming them): one call, the reads are uploaded once and the (sub-batch, part) pairs share one pipeline.
 * The accumulator ends up as n_parts calls of mpn_map_batch_part in the given order would leave it. */
int mpn_map_batch_parts(const mpn_index *const *parts, int32_t n_parts, const mpn_map_opt *opt, int32_t n, const char *const *names,
                        const char *seqs, const int64_t *seq_off, const int32_t *seq_len, const void *r_seqs, const int64_t *r_off,
                        const int32_t *r_len, mpn_hits *acc);
/* out_tags: the strings are made while a part is resident and kept with its hits, so every part of one accumulator is mapped
 * with the same out_tags, and mpn_hits_finish fails (-1) when its opt asks for a tag the accumulated hits do not carry (or for
 * the other cs form).  An accumulator with want_text = 0 computes none.  mpn_hits_export refuses (-1) an accumulator whose hits
 * carry tag strings or =/X CIGARs: the block format does not hold them. */
int64_t mpn_hits_finish(mpn_hits *acc, const mpn_map_opt *opt, int32_t n, const char *const *names, const char *seqs,
                        const char *quals, const int64_t *seq_off, const int32_t *seq_len, char *paf, int64_t paf_cap,
                        mpn_aln_cols *cols);
int32_t mpn_hits_n_parts(const mpn_hits *h);
int32_t mpn_hits_n_seq(const mpn_hits *h);
int32_t mpn_hits_seq_len(const mpn_hits *h, int32_t i);
int32_t mpn_hits_seq_name(const mpn_hits *h, int32_t i, char *buf, int32_t cap);
int64_t mpn_hits_sam_header(const mpn_hits *h, const char *cmdline, char *buf, int64_t cap);

/* ---- index parts sharded over ranks: the hits of a range of reads move from the rank that holds some parts to the rank that owns
 * the reads ----------------------------------------------------------------------------------------------
 * mpn_hits_export: the accumulated (not yet finished) hits of reads [lo, hi) of h as one self-contained byte block: a header (magic,
 * version, k, want_text, n_reads, the exporter's n_seq and n_parts, payload size, checksum), then per read rep_len, the number of hits
 * and each hit's fields, with its CIGAR when want_text.  Only what the merge and the text / column writers read travels.
 * buf == NULL: returns the size needed.  Returns the bytes written, -3 if cap is too small, -1 + mpn_last_error() on bad arguments.
 * mpn_hits_import: append a block to h, which was created for exactly the block's n_reads reads, the way mpn_map_batch_parts would
 * have appended the exporter's parts: every target id shifted by the number of targets h already holds, rep_len = the larger, then the
 * exporter's n_seq targets (names, lens) and n_parts parts added to h.  Blocks of contiguous part blocks imported in part order give
 * what one accumulator over all parts gives.  A block whose k (once h holds a part) or want_text differs from h's, whose read count,
 * target count or part count differs, or that is truncated or corrupted is refused (-1 + mpn_last_error()) and h is left unchanged. */
int64_t mpn_hits_export(const mpn_hits *h, int32_t lo, int32_t hi, void *buf, int64_t cap);
int mpn_hits_import(mpn_hits *h, const void *buf, int64_t len, int32_t n_parts, int32_t n_seq, const char *const *names,
                    const int32_t *lens);

/* After mpn_map_batch(_ex) returned -3 the results of that call are kept by the library (process-wide, until the next
 * mapping call): fetch them with larger buffers instead of mapping the batch again.
 *   mpn_map_fetch_cols: cols->cap rows available; returns the number of rows, -3 if still too small (cols->n_rows = need),
 *                       -1 if nothing is kept.
 *   mpn_map_fetch_text: buf == NULL returns the bytes needed (incl. NUL); otherwise copies the PAF/SAM text and returns
 *                       its length, -3 if cap is too small, -1 if nothing is kept. */
int64_t mpn_map_fetch_cols(mpn_aln_cols *cols);
int64_t mpn_map_fetch_text(char *buf, int64_t cap);

/* Counters and timers of the last mpn_map_batch / mpn_seed_chain_batch on this thread (bench.py roofline line):
 *  [0] input bases  [1] read minimizers  [2] anchors  [3] chains  [4] DP jobs  [5] DP cells  [6] alignments reported
 *  [7] DP rounds    [8] second-pass (exact z-drop) jobs
 * wall-clock ns of the host phases:
 *  [16] H2D reads  [17] seed+chain stage (incl. its kernels)  [18] D2H chains  [19] host: hits from chains
 *  [20] host: plan DP windows  [21] extension stage (H2D jobs, kernels, D2H results)  [22] host: stitch
 *  [23] host: rank/MAPQ/PAF  [24] whole call
 * device ns measured with HIP events on the stream the kernels run on:
 *  [10] sketch  [11] seed lookup+fill  [12] anchor sort  [13] chain DP  [14] chain ends+backtrack
 *  [15] extension DP kernels other than the strip kernel  [25] traceback kernel  [26] z-drop test kernel
 *  inside [21], wall ns: [27] host: kernel choice + scratch layout + staging  [28] enqueue  [29] wait for the GPU
 *  [30] second pass + CIGAR download
 *  [9] device ns of the strip-kernel launches ([15] covers the other DP kernels)  [31] cells (qlen x tlen) those launches computed */
void mpn_map_last_stats(int64_t stats[32]);
/* the same with the slots added after round 1 (returns the number of slots the library has; copies min(n, that)):
 *  [32] sub-batches run (= launches of every per-sub-batch kernel)
 *  device ns of single kernels, HIP events around each launch on its stream:
 *  [33] sketch count pass  [34] sketch fill pass  [35] seed lookup  [36] seed fill  [37] chain DP kernel alone
 *  [38] strip DP <16>  [39] strip DP <32>  [40] strip DP <64>  and their cells [41] [42] [43]
 *  [44] anchors that entered the sort x effective radix passes (bytes moved by the sort = 32 x this)
 *  [45] anchors kept for chaining (segments of at least min_cnt anchors)  [46] device ns of the compaction kernels
 *  device ns of the anchor sort's kernels: [47] partition  [48] chunk sort in LDS  [49] radix passes over the large buckets
 *  [52] device ns of the finishing kernel  [76] device ns of the difference-string kernel's launches (0 unless out_tags asks for text) */
int32_t mpn_map_last_stats_ex(int64_t *stats, int32_t n);

#ifdef __cplusplus
}
#endif
#endif
