// PAF / SAM text of final hits (aln_text.h).
#include "aln_text.h"

#include <stdio.h>
#include <string.h>

namespace mpn {

static double event_identity(const Reg &r) {
    int32_t n_gapo = 0, n_gap = 0;
    for (uint32_t c : r.cigar) { const int32_t op = c & 0xf, len = c >> 4; if (op == 1 || op == 2) { ++n_gapo; n_gap += len; } }
    return (double)r.mlen / (r.blen + r.n_ambi - n_gap + n_gapo);
}

// cs:Z and MD:Z of a hit that has a CIGAR, in this order (both when both were asked for: DESIGN.md section 6)
static void write_diff_tags(const mpn_map_opt *o, const Reg &r, std::string &out) {
    if (r.cigar.empty()) return;
    if (o->out_tags & (MPN_TAG_CS | MPN_TAG_CS_LONG)) { out += "\tcs:Z:"; out += r.cs; }
    if (o->out_tags & MPN_TAG_MD) { out += "\tMD:Z:"; out += r.md; }
}

void write_paf(const Targets mi_, const mpn_map_opt *o, const char *name, int32_t qlen, const std::vector<Reg> &regs, int32_t rep_len,
               std::string &out) {
    const Targets *mi = &mi_;
    char buf[1024];
    for (const Reg &r : regs) {
        const int type = r.id == r.parent ? (r.inv ? 'I' : 'P') : (r.inv ? 'i' : 'S');
        out += name;
        snprintf(buf, sizeof(buf), "\t%d\t%d\t%d\t%c\t", qlen, r.qs, r.qe, "+-"[r.rev]);
        out += buf;
        out += (*mi->names)[r.rid];
        snprintf(buf, sizeof(buf), "\t%d\t%d\t%d\t%d\t%d\t%d", (*mi->lens)[r.rid], r.rs, r.re, r.mlen, r.blen, r.mapq);
        out += buf;
        if (r.has_p) {
            snprintf(buf, sizeof(buf), "\tNM:i:%d\tms:i:%d\tAS:i:%d\tnn:i:%d", r.blen - r.mlen + r.n_ambi, r.dp_max, r.dp_score, r.n_ambi);
            out += buf;
        }
        snprintf(buf, sizeof(buf), "\ttp:A:%c\tcm:i:%d\ts1:i:%d", type, r.cnt, r.score);
        out += buf;
        if (r.parent == r.id) { snprintf(buf, sizeof(buf), "\ts2:i:%d", r.subsc); out += buf; }
        if (r.has_p) {
            const double div = 1.0 - event_identity(r);
            if (div == 0.0) out += "\tde:f:0";
            else { snprintf(buf, sizeof(buf), "\tde:f:%.4f", div); out += buf; }
        }
        if (r.split) { snprintf(buf, sizeof(buf), "\tzd:i:%d", r.split); out += buf; }
        snprintf(buf, sizeof(buf), "\trl:i:%d", rep_len);
        out += buf;
        if (r.has_p && o->with_cigar) {
            out += "\tcg:Z:";
            for (uint32_t c : r.cigar) { snprintf(buf, sizeof(buf), "%d%c", c >> 4, "MIDNSHP=X"[c & 0xf]); out += buf; }
            write_diff_tags(o, r, out);
        }
        out += '\n';
    }
}

static char sam_comp(char c) {
    static const char from[] = "ACGTUNRYKMSWBDHVacgtunrykmswbdhv", to[] = "TGCAANYRMKSWVHDBtgcaanyrmkswvhdb";
    const char *p = c ? strchr(from, c) : nullptr;
    return p ? to[p - from] : c;
}

static void sam_seq(std::string &out, const char *seq, int st, int en, bool rev) {
    if (!rev) out.append(seq + st, (size_t)(en - st));
    else for (int i = en - 1; i >= st; --i) out += sam_comp(seq[i]);
}

// QUAL column of a record whose SEQ is seq[st, en) on strand rev: the qualities in the same orientation, or '*' without them
static void sam_qual(std::string &out, const char *qual, int st, int en, bool rev) {
    out += '\t';
    if (!qual) { out += '*'; return; }
    if (!rev) out.append(qual + st, (size_t)(en - st));
    else for (int i = en - 1; i >= st; --i) out += qual[i];
}

void write_sam(const Targets mi_, const mpn_map_opt *o, const char *name, int32_t qlen, const char *seq, const char *qual,
               const std::vector<Reg> &regs, int32_t rep_len, std::string &out) {
    const Targets *mi = &mi_;
    char buf[1024];
    if (regs.empty()) {
        out += name;
        out += "\t4\t*\t0\t0\t*\t*\t0\t0\t";
        sam_seq(out, seq, 0, qlen, false);
        sam_qual(out, qual, 0, qlen, false);
        snprintf(buf, sizeof(buf), "\trl:i:%d\n", rep_len);
        out += buf;
        return;
    }
    for (size_t i = 0; i < regs.size(); ++i) {
        const Reg &r = regs[i];
        const int type = r.id == r.parent ? (r.inv ? 'I' : 'P') : (r.inv ? 'i' : 'S');
        int flag = r.rev ? 0x10 : 0;
        if (r.parent != r.id) flag |= 0x100;
        else if (!r.sam_pri) flag |= 0x800;
        out += name;
        snprintf(buf, sizeof(buf), "\t%d\t", flag);
        out += buf;
        out += (*mi->names)[r.rid];
        snprintf(buf, sizeof(buf), "\t%d\t%d\t", r.rs + 1, r.mapq);
        out += buf;
        if (!r.has_p) out += '*';
        else {
            const int clip0 = r.rev ? qlen - r.qe : r.qs, clip1 = r.rev ? r.qs : qlen - r.qe;
            const char clip_char = (flag & 0x800) ? 'H' : 'S';
            if (clip0) { snprintf(buf, sizeof(buf), "%d%c", clip0, clip_char); out += buf; }
            for (uint32_t c : r.cigar) { snprintf(buf, sizeof(buf), "%d%c", c >> 4, "MIDNSHP=X"[c & 0xf]); out += buf; }
            if (clip1) { snprintf(buf, sizeof(buf), "%d%c", clip1, clip_char); out += buf; }
        }
        out += "\t*\t0\t0\t";
        if ((flag & 0x900) == 0) { sam_seq(out, seq, 0, qlen, r.rev); sam_qual(out, qual, 0, qlen, r.rev); }
        else if (flag & 0x100) out += "*\t*";
        else { sam_seq(out, seq, r.qs, r.qe, r.rev); sam_qual(out, qual, r.qs, r.qe, r.rev); }
        if (r.has_p) {
            snprintf(buf, sizeof(buf), "\tNM:i:%d\tms:i:%d\tAS:i:%d\tnn:i:%d", r.blen - r.mlen + r.n_ambi, r.dp_max, r.dp_score, r.n_ambi);
            out += buf;
        }
        snprintf(buf, sizeof(buf), "\ttp:A:%c\tcm:i:%d\ts1:i:%d", type, r.cnt, r.score);
        out += buf;
        if (r.parent == r.id) { snprintf(buf, sizeof(buf), "\ts2:i:%d", r.subsc); out += buf; }
        if (r.has_p) {
            const double div = 1.0 - event_identity(r);
            if (div == 0.0) out += "\tde:f:0";
            else { snprintf(buf, sizeof(buf), "\tde:f:%.4f", div); out += buf; }
        }
        if (r.split) { snprintf(buf, sizeof(buf), "\tzd:i:%d", r.split); out += buf; }
        if (r.parent == r.id && r.has_p && regs.size() > 1) {  // SA: the other non-secondary hits that have a CIGAR
            bool any = false;
            for (size_t j = 0; j < regs.size(); ++j) {
                const Reg &q = regs[j];
                if (j == i || q.parent != q.id || !q.has_p) continue;
                if (!any) { out += "\tSA:Z:"; any = true; }
                int l_M, l_I = 0, l_D = 0;
                if (q.qe - q.qs < q.re - q.rs) { l_M = q.qe - q.qs; l_D = (q.re - q.rs) - l_M; }
                else { l_M = q.re - q.rs; l_I = (q.qe - q.qs) - l_M; }
                const int c5 = q.rev ? qlen - q.qe : q.qs, c3 = q.rev ? q.qs : qlen - q.qe;
                out += (*mi->names)[q.rid];
                snprintf(buf, sizeof(buf), ",%d,%c,", q.rs + 1, "+-"[q.rev]);
                out += buf;
                if (c5) { snprintf(buf, sizeof(buf), "%dS", c5); out += buf; }
                if (l_M) { snprintf(buf, sizeof(buf), "%dM", l_M); out += buf; }
                if (l_I) { snprintf(buf, sizeof(buf), "%dI", l_I); out += buf; }
                if (l_D) { snprintf(buf, sizeof(buf), "%dD", l_D); out += buf; }
                if (c3) { snprintf(buf, sizeof(buf), "%dS", c3); out += buf; }
                snprintf(buf, sizeof(buf), ",%d,%d;", q.mapq, q.blen - q.mlen + q.n_ambi);
                out += buf;
            }
        }
        if (r.has_p && o->with_cigar) write_diff_tags(o, r, out);
        snprintf(buf, sizeof(buf), "\trl:i:%d\n", rep_len);
        out += buf;
    }
}

int64_t sam_header_of(const std::vector<std::string> &names, const std::vector<int32_t> &lens, const char *cmdline, char *buf, int64_t cap) {
    std::string h;
    char line[64];
    for (size_t i = 0; i < names.size(); ++i) {
        h += "@SQ\tSN:"; h += names[i];
        snprintf(line, sizeof(line), "\tLN:%d\n", lens[i]);
        h += line;
    }
    h += "@PG\tID:mpn-aligner\tPN:mpn-aligner\tVN:r02";
    if (cmdline && cmdline[0]) { h += "\tCL:"; h += cmdline; }
    h += '\n';
    if ((int64_t)h.size() + 1 > cap) return -3;
    memcpy(buf, h.data(), h.size());
    buf[h.size()] = 0;
    return (int64_t)h.size();
}

}  // namespace mpn
