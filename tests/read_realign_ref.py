"""A serial yardstick for megapath_nano_amd/read_realign.py, the host build of csrc/read_realign_core.h and its kernels: what the
reference's realignment/realign_illumina_reads.py computes, written afresh from DESIGN.md section 6 item 23 with plain lists and
dicts, one record and one position at a time.  It is pinned, byte for byte, by the records the unmodified script printed for the
golden cases (tests/golden/read_realign/, tests/test_read_realign_ref.py).

    realign(lines, contig, ctg_name, min_mq=5, min_coverage=2, consensus=..., realign=..., trace=None) -> the output lines

lines: what `samtools view` prints for the file, without the header; contig: the contig's bases as the FASTA has them.
consensus(ref, reads, bad) -> haplotypes (default: tests/dbg_ref.py, cut to the 200 the script's binding sees);
realign(seqs, positions, cigars, reference, haplotypes, ref_start, ref_prefix, ref_suffix) -> [(position, cigar)] (default:
oracle/realign_oracle.py).  trace: a list that gets one dict per closed chunk: chunk_start; row, the support at chunk_start - 21 ..
chunk_start + 5019; and, unless the chunk is skipped, windows (per split), members (per split and window, the indices of the reads
among the viewed records) and reads (the indices of all reads held at that moment).  A window that starts below 0 is assigned to but
not realigned, as in the product (item 23 h)."""
import string
from collections import Counter

CHUNK, MARGIN = 5000, 20
SPLIT, SPLITS = 1000, 5
JOIN, PAD, WIDEST, DEEPEST = 160, 80, 1000, 1000
COUNT_MAPQ, COUNT_BASEQ, GRAPH_MAPQ, GRAPH_BASEQ = 20, 20, 14, 15
KEEP_BEHIND = MARGIN + WIDEST              # reads whose best position lies further before the chunk than this are written
ALPHABET = string.digits + string.ascii_lowercase + string.ascii_uppercase + '!#$%&()*+./:;<=>?[]^`{|}~'
NAME_LEN = 5


def parse_cigar(text):
    """'3M2D' -> [(3, 'M'), (2, 'D')]; '*' has no number and gives [(0, '*')]"""
    ops, number = [], 0
    for ch in text:
        if ch.isdigit():
            number = 10 * number + int(ch)
        else:
            ops.append((number, ch))
            number = 0
    return ops


def name_of(index):
    """the output name of the record with this index among the viewed records: five digits in base len(ALPHABET), wrapping"""
    index %= len(ALPHABET) ** NAME_LEN
    digits = []
    for _ in range(NAME_LEN):
        index, d = divmod(index, len(ALPHABET))
        digits.append(ALPHABET[d])
    return ''.join(digits[::-1])


def hp_digit(columns):
    """the first column that holds the text HP:i: decides: its sixth character if that is a digit, else nothing"""
    for col in columns:
        if 'HP:i:' in col:
            return col[5] if len(col) > 5 and col[5].isdigit() else None
    return None


def too_clipped(cigar):
    """less than 55 % of the CIGAR's length (plus one) is not soft-clipped"""
    ops = parse_cigar(cigar)
    clipped = sum(n for n, op in ops if op == 'S')
    return 1.0 - float(clipped) / (sum(n for n, _ in ops) + 1) < 0.55


def read_span(seq, cigar):
    """what the script takes for a read's length on the contig: its bases plus its deleted bases"""
    return len(seq) + sum(n for n, op in parse_cigar(cigar) if op == 'D')


def best_window(start, end, windows):
    """the index of the window that [start, end) overlaps most, the first of equals; None without an overlap"""
    best, at = 0, None
    for k, (a, b) in enumerate(windows):
        shared = min(end, b) - max(start, a)
        if shared > best:
            best, at = shared, k
    return at


def indel_score(cigar):
    return sum(n for n, op in parse_cigar(cigar) if op in 'ID')


def record_of(line, index):
    col = line.strip().split()                      # (any white space separates: an aux value with a blank is several columns)
    rec = dict(index=index, name=name_of(index), flag=col[1], pos=int(col[3]) - 1, mapq=int(col[4]), cigar=col[5], rnext=col[6], pnext=col[7],
               seq=col[9].upper(), qual_text=col[10], qual=[ord(c) - 33 for c in col[10]], hp=hp_digit(col[11:]))
    rec['end'] = rec['pos'] + read_span(rec['seq'], rec['cigar'])
    rec['best'] = (rec['pos'], rec['cigar'], None)           # position, CIGAR, indel score of the best realignment so far
    return rec


def add_support(rec, contig, chunk_start, support):
    """the positions at which this record disagrees with the contig, added to `support`"""
    ref_at, read_at = rec['pos'], 0
    in_region = lambda p: chunk_start - MARGIN <= p <= chunk_start + CHUNK + MARGIN
    for n, op in parse_cigar(rec['cigar']):
        if op == '=':
            ref_at, read_at = ref_at + n, read_at + n
        elif op in 'MX':
            for k in range(n):
                if rec['qual'][read_at + k] >= COUNT_BASEQ:
                    base = contig[ref_at + k]
                    if base in 'ACGT' and base != rec['seq'][read_at + k]:
                        support[ref_at + k] += 1
            ref_at, read_at = ref_at + n, read_at + n
        elif op in 'IS':
            before = contig[ref_at - 1]                      # (at position 0: the contig's last base)
            clean = all(q >= COUNT_BASEQ for q in rec['qual'][read_at:read_at + n])
            if in_region(ref_at) and before in 'ACGT' and clean:
                for p in range(ref_at - n, ref_at + n):
                    support[p] += 1
            read_at += n
        elif op == 'D':
            if in_region(ref_at) and contig[ref_at - 1] in 'ACGT':
                for p in range(ref_at, ref_at + n):
                    support[p] += 1
            ref_at += n
        # N, H and P: nothing moves


def windows_of(positions):
    """ascending candidate positions -> windows: a run is joined while the next position is at most JOIN behind the last, then padded"""
    runs = []
    for p in positions:
        if runs and p <= runs[-1][1] + JOIN:
            runs[-1][1] = p
        else:
            runs.append([p, p])
    return [(a - PAD, b + PAD) for a, b in runs]


def accept(rec, position, cigar):
    """one realignment result against the best so far"""
    cigar = cigar.replace('X', 'M')
    if (position, cigar) == (rec['pos'], rec['cigar']):
        return
    best_pos, best_cigar, best_score = rec['best']
    if best_score and (position, cigar) == (best_pos, best_cigar):
        return
    score = indel_score(cigar)
    if not best_score or score >= best_score:                # (a best score of 0 counts as none)
        rec['best'] = (position, cigar, score)


def output_line(rec, ctg_name):
    tail = 'HP:i:' + rec['hp'] if rec['hp'] else ''
    return '\t'.join([rec['name'], rec['flag'], ctg_name, str(rec['best'][0] + 1), str(rec['mapq']), rec['best'][1], rec['rnext'], rec['pnext'],
                      rec['pnext'], rec['seq'], rec['qual_text'], tail]) + '\n'


def _default_consensus(ref, reads, bad):
    import dbg_ref
    return dbg_ref.get_consensus(ref, reads, bad)[0][:200]


def _default_realign(*args):
    from oracle import realign_oracle
    return realign_oracle.realign_reads(*args)


def realign_window(window, names, held, contig, consensus, realign_reads):
    """the reads `names` of one window through consensus and realigner; their results go to accept()"""
    start, end = window
    reads = [held[n] for n in names]
    graph = [r for r in reads if r['mapq'] >= GRAPH_MAPQ and not (r['pos'] > end or r['end'] < start)]
    haplotypes = consensus(contig[start:end], [r['seq'] for r in graph], [[k for k, q in enumerate(r['qual']) if q < GRAPH_BASEQ] for r in graph])
    if not haplotypes or haplotypes == [contig[start:end]] or not reads:
        return
    left = max(0, min(min(r['pos'] for r in reads), start) - MARGIN)
    right = max(max(r['end'] for r in reads), end) + MARGIN
    prefix, suffix = contig[left:start], contig[end:right]
    some = reads[:DEEPEST]
    results = realign_reads([r['seq'] for r in some], [r['pos'] for r in some], [r['cigar'] for r in some], prefix + contig[start:end] + suffix,
                            [prefix + h + suffix for h in haplotypes], left, len(prefix), len(suffix))
    for r, (position, cigar) in zip(some, results):
        if cigar != '' and (position, cigar) != (r['pos'], r['cigar']):
            accept(r, position, cigar)


def realign(lines, contig, ctg_name, min_mq=5, min_coverage=2, consensus=None, realign=None, trace=None):
    consensus, realign_reads = consensus or _default_consensus, realign or _default_realign
    contig = contig.upper()
    viewed = [l for l in lines if l.split('\t')[2] == ctg_name and not (min_mq > 0 and int(l.split('\t')[4]) < min_mq)]     # samtools view -q
    out, held, support = [], {}, Counter()         # held: name -> record, in the order the records came

    def close_chunk(chunk_start):
        lo, hi = chunk_start - MARGIN - 1, chunk_start + CHUNK + MARGIN - 1
        candidates = sorted(p for p, n in support.items() if n >= min_coverage and lo <= p <= hi)
        entry = None
        if trace is not None:
            entry = dict(chunk_start=chunk_start, row=[support.get(p, 0) for p in range(lo, hi + 1)], windows=None, members=None, reads=None)
            trace.append(entry)
        if not held or not candidates:
            return                                 # (nothing is written either)
        if entry is not None:
            entry.update(windows=[], members=[], reads=[r['index'] for r in held.values()])
        for s in range(SPLITS):
            a = chunk_start + s * SPLIT - MARGIN - 1
            windows = windows_of([p for p in candidates if a <= p < a + SPLIT + 2 * MARGIN + 1])
            of_window = [[] for _ in windows]
            if windows:
                last_end = max(b for _, b in windows)
                for name, r in held.items():
                    k = best_window(r['pos'], r['end'], windows) if r['pos'] <= last_end else None
                    if k is not None:
                        of_window[k].append(name)
            if entry is not None:
                entry['windows'].append(windows)
                entry['members'].append([[held[n]['index'] for n in names] for names in of_window])
            for window, names in zip(windows, of_window):
                if window[1] - window[0] <= WIDEST and window[0] >= 0:
                    realign_window(window, names, held, contig, consensus, realign_reads)
        limit = chunk_start - KEEP_BEHIND
        for r in sorted(held.values(), key=lambda r: r['best'][0]):         # (stable: equal positions stay in arrival order)
            if r['best'][0] < limit:
                out.append(output_line(r, ctg_name))
                del held[r['name']]
        for p in [p for p in support if p < limit]:
            del support[p]

    chunk_start = None
    for index, line in enumerate(viewed):
        rec = record_of(line, index)
        if chunk_start is None:
            chunk_start = rec['pos']
        if rec['pos'] >= chunk_start + CHUNK + MARGIN:       # one chunk is closed and one step taken, however far ahead the record is
            close_chunk(chunk_start)
            chunk_start += CHUNK
        if rec['cigar'] == '*' or too_clipped(rec['cigar']):
            continue
        held[rec['name']] = rec
        if rec['mapq'] >= COUNT_MAPQ:
            add_support(rec, contig, chunk_start, support)
    if chunk_start is not None:
        close_chunk(chunk_start)
    out += [output_line(r, ctg_name) for r in sorted(held.values(), key=lambda r: r['best'][0])]
    return out
