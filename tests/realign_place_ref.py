"""Plain restatement of the amplicon realigner's placement stage: BuildIndex + FastAlignReadsToHaplotype + FastAlignStrings
(realigner.cpp:147-253, 429-451) written out literally -- a dict from 32-mer to its (read, offset) occurrences in insertion order,
the loop over haplotype positions, start = max(0, i - offset), the fit test, the `position == start` skip, the N rule, coverage
counters and the drop test with its unsigned subtraction -- and recording what realigner.place_batch (mpn_realign_place_batch)
returns.  tests/test_realign_place_ref.py pins it to oracle.realign_oracle.fast_align_reads_to_haplotypes.

The reference leaves a haplotype's loop at the first position that fails the coverage test.  The placement stage lists the
placements of the whole haplotype, so the loop here goes on behind that position, only to list: the haplotype's results are
taken at the moment the reference returns."""

KMER = 32
MAX_MM = 2
MATCH, MISMATCH = 4, 6
NOT_ALIGNED = -1


def fast_align_strings(s1, s2, max_mismatches):
    """FastAlignStrings (realigner.cpp:232-253) -> (score, mismatches)"""
    matches = mismatches = 0
    for i in range(len(s1)):
        c1, c2 = s1[i], s2[i]
        if c1 != c2 and (c1 != 'N' and c2 != 'N'):
            mismatches += 1
            if mismatches == max_mismatches:
                return 0, mismatches
        else:
            matches += 1
    return matches * MATCH - mismatches * MISMATCH, mismatches


def build_index(seqs):
    """BuildIndex (realigner.cpp:429-451): reads of 32 bases or fewer are not indexed"""
    index = {}
    for rid, read in enumerate(seqs):
        if len(read) <= KMER:
            continue
        for i in range(len(read) - KMER + 1):
            index.setdefault(read[i:i + KMER], []).append((rid, i))
    return index


def place_window(seqs, reference, haplotypes, ref_prefix, ref_suffix, **_):
    """One window -> dict(hits, kmer, dropped, score, position, read_score, evals):
    hits        [(hap, read, start, mm, t, p)]: the first accepted evaluation of every (haplotype, read, start), in the order the
                reference evaluates (haplotype, t, read, p)
    kmer        per haplotype: bytes, 1 at every position 0 .. HL - 32 whose 32-mer is in the index
    dropped, score          per haplotype
    position, read_score    per haplotype, per read
    evals       [(hap, t, read, p, start, mm or None)]: every index occurrence looked at (mm None: the read does not fit there);
                for the cases' own assertions"""
    index = build_index(seqs)
    out = dict(hits=[], kmer=[], dropped=[], score=[], position=[], read_score=[], evals=[])
    for hi, hap in enumerate(haplotypes):
        assert len(hap) >= KMER
        cache = {}
        position = [NOT_ALIGNED] * len(seqs)
        score = [0] * len(seqs)
        hap_score = 0
        is_ref = hap == reference
        coverage = [0] * len(hap)
        kmer = bytearray(len(hap) - KMER + 1)
        listed = set()
        result = None            # (dropped, hap_score, positions, scores) once the reference has returned
        for i in range(len(hap) - KMER + 1):
            occs = index.get(hap[i:i + KMER])
            if occs is None:
                continue
            kmer[i] = 1
            for rid, rpos in occs:
                start = max(0, i - rpos)
                size = len(seqs[rid])
                if start + size > len(hap):
                    out['evals'].append((hi, i, rid, rpos, start, None))
                    continue
                if (rid, start) not in cache:
                    cache[(rid, start)] = fast_align_strings(hap[start:start + size], seqs[rid], MAX_MM + 1)
                sc, mm = cache[(rid, start)]
                out['evals'].append((hi, i, rid, rpos, start, mm))
                if mm <= MAX_MM and (rid, start) not in listed:
                    listed.add((rid, start))
                    out['hits'].append((hi, rid, start, mm, i, rpos))
                if position[rid] != NOT_ALIGNED and position[rid] == start:
                    continue
                if mm <= MAX_MM:
                    old = score[rid]
                    for pos in range(start, start + size):
                        coverage[pos] += 1
                    if old < sc:
                        score[rid] = sc
                        hap_score -= old
                        hap_score += sc
                        position[rid] = start
            # i < haplotype.size() - ref_suffix_len_ is a comparison of size_t values
            if result is None and coverage[i] == 0 and i >= ref_prefix and i < (len(hap) - ref_suffix) % (1 << 64) and not is_ref:
                result = (True, 0, None, None)
        if result is None:
            result = (False, hap_score, position, score)
        dropped, hap_score, position, score = result
        if hap_score == 0:
            position, score = [NOT_ALIGNED] * len(seqs), [0] * len(seqs)
        out['kmer'].append(bytes(kmer))
        out['dropped'].append(dropped)
        out['score'].append(hap_score)
        out['position'].append(list(position))
        out['read_score'].append(list(score))
    return out


RESULT_KEYS = ('hits', 'kmer', 'dropped', 'score', 'position', 'read_score')


def results(placed):
    """what place_batch returns for the window"""
    return {k: placed[k] for k in RESULT_KEYS}
