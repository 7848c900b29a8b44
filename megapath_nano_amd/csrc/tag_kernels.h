// Difference strings of finished alignments on the GPU: the cs tag (short and long form), the MD tag and the =/X CIGAR of
// --eqx, from the fixed CIGAR, the read and the 2-bit target while all three are resident (the host keeps no copy of the
// targets, and a streamed index part is gone by the time text is written).  Launched after aln_finish_wave_kernel, and only
// when a caller asked for one of the outputs.
#pragma once
#include "fin_kernels.h"

namespace mpn {

enum { TAG_CS = 1, TAG_CS_LONG = 2, TAG_MD = 4, TAG_EQX = 8 };

struct TagOut { int64_t cs_off, md_off, eqx_off; int32_t cs_len, md_len, n_eqx, pad; };
// cursors of the three output pools, and the flag a write past a pool or past an alignment's own slice sets
enum { TAGC_CS = 0, TAGC_MD = 1, TAGC_EQX = 2, TAGC_OVERFLOW = 3, TAGC_N = 4 };

__device__ __forceinline__ int tag_hb(unsigned long long m, int L) {   // highest set bit of m below bit L, or -1
    const unsigned long long x = L >= 64 ? m : m & ((1ULL << L) - 1);
    return x ? 63 - __clzll((long long)x) : -1;
}
__device__ __forceinline__ unsigned long long tag_below(int L) { return L >= 64 ? ~0ULL : (1ULL << L) - 1; }
__device__ __forceinline__ int tag_ndig(uint32_t v) {
    return v < 10u ? 1 : v < 100u ? 2 : v < 1000u ? 3 : v < 10000u ? 4 : v < 100000u ? 5 : v < 1000000u ? 6 : v < 10000000u ? 7 : v < 100000000u ? 8 : v < 1000000000u ? 9 : 10;
}
__device__ __forceinline__ void tag_put_num(char *p, uint32_t v, int nd) { for (int i = nd - 1; i >= 0; --i) { p[i] = (char)('0' + v % 10u); v /= 10u; } }

// One wave per alignment.  The op start positions (column, read, target) come from a scan over the op lengths and stay in
// LDS (IN_LDS) or in global scratch (CIGARs beyond the LDS classes).  The alignment's columns are then taken 64 at a time:
// a lane finds its column's op by a bounded binary search, loads the aligned word that holds its read base and the 2-bit
// word that holds its target base, and one ballot each gives the match / mismatch / op-start masks of the chunk.  Everything
// that is a run -- the count of a cs ":k", the MD counter (which runs across insertions and chunks), the length of an = or X
// op -- is written by the lane of the column that ENDS the run (the first column that does not continue it; the column one
// past the end of the alignment closes what is still open), from the masks by bit scans plus a carry from the earlier chunks.
// A lane's byte and op counts go through a wave prefix scan to its store offsets.  The chunks are walked twice: a counting
// walk sizes the three outputs exactly, lane 0 takes the slices from the pools' cursors, the second walk stores.
template <bool IN_LDS>
__global__ __launch_bounds__(64) void aln_tags_wave_kernel(const FinJob *__restrict__ jobs, const FinOut *__restrict__ fouts, const int32_t *__restrict__ list,
                                                           int n_list, const uint32_t *__restrict__ CIG, int32_t *__restrict__ POS,
                                                           const uint8_t *__restrict__ reads, const int64_t *__restrict__ read_off,
                                                           const int32_t *__restrict__ read_len, RefView rv, int tags, char *__restrict__ CS, long long cs_cap,
                                                           char *__restrict__ MD, long long md_cap, uint32_t *__restrict__ EQX, long long eqx_cap,
                                                           unsigned long long *__restrict__ cursors, TagOut *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t tag_lds[];
    const int lane = threadIdx.x;
    auto sync = []() { if constexpr (IN_LDS) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); else __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent"); __builtin_amdgcn_wave_barrier(); };
    auto incl_scan = [&](int v) { int x = v; for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(x, d); if (lane >= d) x += o; } return x; };
    const bool want_cs = (tags & (TAG_CS | TAG_CS_LONG)) != 0, cs_long = (tags & TAG_CS_LONG) != 0, want_md = (tags & TAG_MD) != 0, want_eqx = (tags & TAG_EQX) != 0;
    for (int li = blockIdx.x; li < n_list; li += gridDim.x) {
        const int jid = list[li];
        const FinJob jb = jobs[jid];
        const FinOut fo = fouts[jid];
        const uint32_t *cg = CIG + jb.cig_off;
        const int n = fo.n_cigar;
        int32_t *colS = IN_LDS ? reinterpret_cast<int32_t *>(tag_lds) : POS + 3 * jb.cig_off;
        int32_t *qS = colS + n, *tS = qS + n;
        const int64_t roff = read_off[jb.read];
        const int32_t rlen = read_len[jb.read];
        const int qs = jb.qs1 + fo.qshift;                       // the finished alignment may start later than the job says
        const int64_t g0 = rv.seq_off[jb.rid] + jb.rs1 + fo.tshift;
        // ---- op start positions by scan ----
        int ncol = 0, tspan = 0;
        {
            const int per = (n + 63) / 64, k_lo = min(n, lane * per), k_hi = min(n, k_lo + per);
            int ca = 0, qa = 0, ta = 0;
            for (int k = k_lo; k < k_hi; ++k) { const uint32_t op = cg[k] & 0xf, len = cg[k] >> 4; ca += len; qa += op != 2 ? len : 0; ta += op != 1 ? len : 0; }
            const int ci = incl_scan(ca), qi = incl_scan(qa), ti = incl_scan(ta);
            int c = ci - ca, q = qi - qa, t = ti - ta;
            for (int k = k_lo; k < k_hi; ++k) {
                const uint32_t op = cg[k] & 0xf, len = cg[k] >> 4;
                colS[k] = c; qS[k] = q; tS[k] = t;
                c += len; q += op != 2 ? len : 0; t += op != 1 ? len : 0;
            }
            ncol = __shfl(ci, 63); tspan = __shfl(ti, 63);
        }
        // ambiguous-base runs of the target that overlap the interval (rare): [run_lo, run_hi)
        int run_lo = 0, run_hi = 0;
        if (rv.n_runs > 0 && tspan > 0) {
            int lo = 0, hi = rv.n_runs;  // first run that ends after g0
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (rv.nrun_e[mid] <= g0) lo = mid + 1; else hi = mid; }
            run_lo = lo;
            hi = rv.n_runs;              // first run that starts at or after the interval's end
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (rv.nrun_s[mid] < g0 + tspan) lo = mid + 1; else hi = mid; }
            run_hi = lo;
        }
        sync();
        int64_t cs_base = 0, md_base = 0, eqx_base = 0;
        int cs_tot = 0, md_tot = 0, eqx_tot = 0;
        bool ok = true;
        for (int pass = 0; pass < 2 && ok; ++pass) {
            const bool wr = pass == 1;
            int cs_pos = 0, md_pos = 0, eqx_pos = 0;     // what the earlier chunks produced
            int carry_cs = 0, carry_md = 0, carry_e = 0;  // open cs run, MD counter, open =/X run at the end of the previous chunk
            int prev_m = 0, prev_match = 0;               // the previous chunk's last column: inside an M op; matching
            int kbase = 0;                                // op of the previous chunk's last column
            for (int c0 = 0; c0 <= ncol; c0 += 64) {
                const int c = c0 + lane;
                const bool valid = c < ncol, term = c == ncol;
                int k = 0, kind = 3, qc = 4, tc = 4;
                uint32_t opw = 0;
                bool first = false;
                if (valid) {
                    int lo = kbase, hi = min(n - 1, kbase + 64);   // no op is empty: 64 columns span at most 64 more ops
                    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (colS[mid] <= c) lo = mid; else hi = mid - 1; }
                    k = lo;
                    opw = cg[k];
                    kind = (int)(opw & 0xf);
                    const int j = c - colS[k];
                    first = j == 0;
                    if (kind != 2) {   // the aligned 4-byte word around the read base (the reads buffer is padded for it)
                        const int p = qs + qS[k] + j;
                        const int64_t a = roff + (jb.rev ? rlen - 1 - p : p);
                        const uint32_t w = *reinterpret_cast<const uint32_t *>(reads + (a & ~(int64_t)3));
                        const int x = nt4_code((uint8_t)(w >> (8 * (int)(a & 3))));
                        qc = jb.rev ? (x < 4 ? 3 - x : 4) : x;
                    }
                    if (kind != 1) {
                        const int64_t g = g0 + tS[k] + j;
                        tc = (int)(rv.seq2[g >> 4] >> (2 * (int)(g & 15)) & 3u);
                        if (run_hi > run_lo) {   // last run with start <= g
                            int lo2 = run_lo, hi2 = run_hi;
                            while (lo2 < hi2) { const int mid = (lo2 + hi2) >> 1; if (rv.nrun_s[mid] <= g) lo2 = mid + 1; else hi2 = mid; }
                            if (lo2 > run_lo && g < rv.nrun_e[lo2 - 1]) tc = 4;
                        }
                    }
                }
                const bool isM = kind == 0, isI = kind == 1, isD = kind == 2;
                const bool mt = isM && qc == tc, mm = isM && qc != tc;
                const unsigned long long Mt = __ballot(mt), Mm = __ballot(mm), F = __ballot(first), Dm = __ballot(isD);
                const unsigned long long Mop = Mt | Mm, low = tag_below(lane);
                const bool active = valid || term;
                const bool before_mt = lane > 0 ? (Mt >> (lane - 1) & 1) != 0 : carry_cs > 0;
                // ---- cs ----
                int cs_n = 0, cs_run = 0;
                bool cs_flush = false, cs_start = false;
                if (want_cs) {
                    const unsigned long long S = Mt & (F | ~(Mt << 1 | (carry_cs > 0 ? 1ULL : 0ULL)));   // columns that open a run of matches
                    cs_start = (S >> lane & 1) != 0;
                    const int own = mm ? 3 : (isI || isD) ? 1 + (first ? 1 : 0) : 0;
                    if (cs_long) cs_n = mt ? 1 + (cs_start ? 1 : 0) : own;
                    else {
                        cs_flush = active && before_mt && !(mt && !first);
                        if (cs_flush) { const int p = tag_hb(S, lane); cs_run = p >= 0 ? lane - p : lane + carry_cs; }
                        cs_n = (cs_flush ? 1 + tag_ndig((uint32_t)cs_run) : 0) + own;
                    }
                    if (Mt >> 63 & 1) { const int p = tag_hb(S, 64); carry_cs = p >= 0 ? 64 - p : carry_cs + 64; } else carry_cs = 0;
                }
                // ---- MD ----
                int md_n = 0, md_cnt = 0;
                const bool md_emit = mm || (isD && first) || term;
                if (want_md) {
                    const unsigned long long R = Mm | Dm;   // columns that reset the counter
                    if (md_emit) {
                        const int p = tag_hb(R, lane);
                        md_cnt = p >= 0 ? __popcll(Mt & low & ~tag_below(p + 1)) : __popcll(Mt & low) + carry_md;
                        md_n = tag_ndig((uint32_t)md_cnt) + (mm ? 1 : isD ? 2 : 0);
                    } else if (isD) md_n = 1;
                    const int p = tag_hb(R, 64);
                    carry_md = p >= 0 ? __popcll(Mt & ~tag_below(p + 1)) : carry_md + __popcll(Mt);
                }
                // ---- =/X ops ----
                int e_n = 0, e_run = 0;
                const int prev_match_in = prev_match;
                bool e_flush = false;
                if (want_eqx) {
                    const unsigned long long E = Mop & (F | ~(Mop << 1 | (unsigned long long)prev_m) | (Mt ^ (Mt << 1 | (unsigned long long)prev_match)));   // columns that open an = or X op
                    const bool before_m = lane > 0 ? (Mop >> (lane - 1) & 1) != 0 : prev_m != 0;
                    e_flush = active && before_m && (!isM || (E >> lane & 1));
                    if (e_flush) { const int p = tag_hb(E, lane); e_run = p >= 0 ? lane - p : lane + carry_e; }
                    e_n = (e_flush ? 1 : 0) + ((isI || isD) && first ? 1 : 0);
                    if (Mop >> 63 & 1) { const int p = tag_hb(E, 64); carry_e = p >= 0 ? 64 - p : carry_e + 64; prev_m = 1; prev_match = (int)(Mt >> 63 & 1); }
                    else { carry_e = 0; prev_m = 0; prev_match = 0; }
                }
                const int cs_i = incl_scan(cs_n), md_i = incl_scan(md_n), e_i = incl_scan(e_n);
                if (wr) {
                    if (cs_n) {
                        const int o = cs_pos + cs_i - cs_n;
                        if (o + cs_n > cs_tot) cursors[TAGC_OVERFLOW] = 1;
                        else {
                            char *p = CS + cs_base + o;
                            if (cs_flush) { *p++ = ':'; const int nd = tag_ndig((uint32_t)cs_run); tag_put_num(p, (uint32_t)cs_run, nd); p += nd; }
                            if (mt) { if (cs_long) { if (cs_start) *p++ = '='; *p = "ACGTN"[tc]; } }
                            else if (mm) { p[0] = '*'; p[1] = "acgtn"[tc]; p[2] = "acgtn"[qc]; }
                            else if (isI) { if (first) *p++ = '+'; *p = "acgtn"[qc]; }
                            else if (isD) { if (first) *p++ = '-'; *p = "acgtn"[tc]; }
                        }
                    }
                    if (md_n) {
                        const int o = md_pos + md_i - md_n;
                        if (o + md_n > md_tot) cursors[TAGC_OVERFLOW] = 1;
                        else {
                            char *p = MD + md_base + o;
                            if (md_emit) { const int nd = tag_ndig((uint32_t)md_cnt); tag_put_num(p, (uint32_t)md_cnt, nd); p += nd; if (isD) *p++ = '^'; }
                            if (mm || isD) *p = "ACGTN"[tc];
                        }
                    }
                    if (e_n) {
                        const int o = eqx_pos + e_i - e_n;
                        if (o + e_n > eqx_tot) cursors[TAGC_OVERFLOW] = 1;
                        else {
                            uint32_t *p = EQX + eqx_base + o;
                            if (e_flush) *p++ = (uint32_t)e_run << 4 | ((lane > 0 ? (Mt >> (lane - 1) & 1) != 0 : prev_match_in != 0) ? 7u : 8u);
                            if ((isI || isD) && first) *p = opw;
                        }
                    }
                }
                cs_pos += __shfl(cs_i, 63); md_pos += __shfl(md_i, 63); eqx_pos += __shfl(e_i, 63);
                kbase = __shfl(k, 63);
            }
            if (!wr) {   // the slices, exactly as large as the counting walk found them
                cs_tot = cs_pos; md_tot = md_pos; eqx_tot = eqx_pos;
                unsigned long long b0 = 0, b1 = 0, b2 = 0;
                if (lane == 0) {
                    if (cs_tot) b0 = atomicAdd(&cursors[TAGC_CS], (unsigned long long)cs_tot);
                    if (md_tot) b1 = atomicAdd(&cursors[TAGC_MD], (unsigned long long)md_tot);
                    if (eqx_tot) b2 = atomicAdd(&cursors[TAGC_EQX], (unsigned long long)eqx_tot);
                }
                cs_base = (int64_t)__shfl(b0, 0); md_base = (int64_t)__shfl(b1, 0); eqx_base = (int64_t)__shfl(b2, 0);
                if (cs_base + cs_tot > cs_cap || md_base + md_tot > md_cap || eqx_base + eqx_tot > eqx_cap) {
                    ok = false;
                    if (lane == 0) cursors[TAGC_OVERFLOW] = 1;
                }
            }
        }
        if (lane == 0) {
            TagOut o;
            o.cs_off = cs_base; o.md_off = md_base; o.eqx_off = eqx_base;
            o.cs_len = ok ? cs_tot : 0; o.md_len = ok ? md_tot : 0; o.n_eqx = ok ? eqx_tot : 0; o.pad = 0;
            out[jid] = o;
        }
        sync();
    }
}

}  // namespace mpn
