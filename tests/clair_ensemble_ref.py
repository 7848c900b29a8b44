"""A plain restatement (test infrastructure) of the two post-processing steps of the reference's ensemble chain, in Python floats
and strings only: clair/post_processing/ensemble.py (ensemble_text) and clair/post_processing/overlap_variant.py (overlap_text).
tests/test_clair_ensemble_ref.py holds it against what the reference's own scripts printed (tests/golden/clair_ensemble/)."""

CELLS = 33 * 8 * 4


def ensemble_text(text, minimum_count=0):
    """the lines of --output_for_ensemble, concatenated over resamples and models -> what ensemble.py prints"""
    order, count, first_seq, cells, sums = [], {}, {}, {}, {}
    for row in text.splitlines(keepends=True):
        col = row.split('\t')
        key = (col[0], col[1])                                    # strings: '9' and '09' are two sites
        ints = [int(v) for v in col[3:3 + CELLS]]
        ps = [float(v) for v in col[3 + CELLS:]]                   # (the last one carries the newline; float() strips it)
        if key not in count:
            order.append(key)
            count[key], first_seq[key], cells[key], sums[key] = 1, col[2], ints, ps
        else:
            count[key] += 1
            cells[key] = [a + b for a, b in zip(cells[key], ints)]
            sums[key] = [a + b for a, b in zip(sums[key], ps)]     # float64, in input order
    out = []
    for key in order:
        n = count[key]
        if n < minimum_count:
            continue
        out.append('\t'.join([key[0], key[1], first_seq[key], '\t'.join(str(v) for v in cells[key]),
                              '\t'.join('{:.6f}'.format(p / n) for p in sums[key])]) + '\n')
    return ''.join(out)


def _record(row):
    col = row.split('\t')
    alts = col[4].split(',')
    sample = col[-1].split(':')
    return dict(chrom=col[0], pos=int(col[1]), ref=col[3], alt=alts[0], alt2=alts[1] if len(alts) > 1 else None, qual=int(float(col[5])),
                gt=sample[0], dp=sample[2], af=sample[3])


def _deletion(r):
    """the half-open 0-based interval the longest deletion of a record covers, anchor base included; None: no deletion"""
    n = len(r['ref']) - min(len(r['alt']), 1024 if r['alt2'] is None else len(r['alt2']))
    return (r['pos'] - 1, r['pos'] + n) if n > 0 else None


def _snp(r):
    same = len(r['ref']) == len(r['alt']) or (r['alt2'] is not None and len(r['ref']) == len(r['alt2']))
    return (r['pos'] - 1, r['pos']) if same else None


def _inside(a, b):
    return a is not None and b is not None and a[0] <= b[0] < a[1]


def overlaps(r1, r2):
    if r1['chrom'] != r2['chrom']:
        return False
    if r1['pos'] > r2['pos']:
        r1, r2 = r2, r1
    return _inside(_deletion(r1), _snp(r2)) or _inside(_deletion(r1), _deletion(r2))


def overlap_text(text):
    """a sorted VCF -> what overlap_variant.py prints"""
    rows = [r[:-1] for r in text.splitlines(keepends=True)]       # (the script cuts one character off every row)
    head = [r for r in rows if r[0] == '#']
    kept = []
    for r in (_record(r) for r in rows if r[0] != '#'):
        if kept and overlaps(kept[-1], r):
            if kept[-1]['qual'] > r['qual']:
                continue
            kept.pop()
        kept.append(r)
    body = ['\t'.join([r['chrom'], str(r['pos']), '.', r['ref'], r['alt'] + (',' + r['alt2'] if r['alt2'] is not None else ''), str(r['qual']), '.', '.',
                       'GT:GQ:DP:AF', ':'.join([r['gt'], str(r['qual']), r['dp'], r['af']])]) for r in kept]
    return ''.join(r + '\n' for r in head + body)
