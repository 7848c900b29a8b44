// Text of final hits: PAF lines, SAM records and the SAM header (minimap2 2.17's writers for single-segment reads).
// Host only: no HIP include.
#pragma once
#include "hit_host.h"

#include <string>
#include <vector>

namespace mpn {

// names and lengths of the targets the hits refer to: one index, or all parts of a split index in order
struct Targets {
    const std::vector<std::string> *names;
    const std::vector<int32_t> *lens;
};

void write_paf(const Targets mi_, const mpn_map_opt *o, const char *name, int32_t qlen, const std::vector<Reg> &regs, int32_t rep_len,
               std::string &out);
// SAM records of one read (minimap2 2.17 -a: mm_write_sam3 / write_sam_cigar / sam_write_sq for single-segment reads
// without read group).  A read without hits gets a flag-4 record; qual may be null (QUAL is then '*').
void write_sam(const Targets mi_, const mpn_map_opt *o, const char *name, int32_t qlen, const char *seq, const char *qual,
               const std::vector<Reg> &regs, int32_t rep_len, std::string &out);
// "@SQ" lines of the targets + one "@PG" line (cmdline may be null); returns the text length, or -3 if cap is too small
int64_t sam_header_of(const std::vector<std::string> &names, const std::vector<int32_t> &lens, const char *cmdline, char *buf, int64_t cap);

}  // namespace mpn
