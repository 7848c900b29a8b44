"""Cases and brute-force statements shared by tests/test_assembly_selection.py (CPU), tests/test_assembly_selection_gpu.py and
tests/golden/make_assembly_selection_golden.py: the good rows of a read (mpn_good_rows), grouped sums (mpn_sum_by_key) in plain
loops over dicts, and the seeded tables behind good_align_list, align_stat_by_sequence_id and assembly_selection.  Built on the
generators of tests/best_cases.py."""
import json
import os

import numpy as np
import pandas as pd

from best_cases import ASSEMBLIES, BELOW_ONE, LENGTHS, TINY, best_table, noise_bed_for, table_digest

TILE = 2048            # MPN_BEST_TILE (tests/test_assembly_selection.py checks it against the package's number)
TOP = 2 ** 32 - 1      # the largest value of a summed column


# ---- brute force ---------------------------------------------------------------------------------------------------------------
def brute_good_rows(read, unit, score, tiebreak, n_reads, threshold):
    """-> good_row, read_best as lists.  threshold None: every kept row."""
    kept = {}
    for i in range(len(read)):
        key = (int(read[i]), int(unit[i]))
        j = kept.get(key)
        if j is None or (int(score[i]), float(tiebreak[i])) >= (int(score[j]), float(tiebreak[j])):   # a later equal row replaces
            kept[key] = i
    best = {}
    for (r, _), i in kept.items():
        best[r] = max(best.get(r, int(score[i])), int(score[i]))
    good = [kept[k] for k in sorted(kept) if threshold is None or float(int(score[kept[k]])) >= float(best[k[0]]) * float(threshold)]
    return good, [best.get(r, 0) for r in range(n_reads)]


def brute_sum_by_key(key, n_keys, cols):
    """-> count, sums[c][k] as lists of Python ints"""
    count, sums = [0] * n_keys, [[0] * n_keys for _ in cols]
    key = [int(k) for k in key]
    for k in key:
        count[k] += 1
    for c, col in enumerate(cols):
        row = sums[c]
        for k, v in zip(key, col.tolist()):
            row[k] += v
    return count, sums


# ---- cases for mpn_good_rows ---------------------------------------------------------------------------------------------------
def _rows(read, unit, score, tiebreak, n_reads, n_units, threshold):
    return dict(read=np.asarray(read, np.int32), unit=np.asarray(unit, np.int32), score=np.asarray(score, np.int64),
                tiebreak=np.asarray(tiebreak, np.float64), n_reads=int(n_reads), n_units=int(n_units), threshold=threshold)


def _seeded(rng, n, n_reads, n_units, threshold, base=500, spread=4):
    """about n / n_reads rows a read, scores from `spread` adjacent values, tiebreakers that repeat (so whole rows tie), the largest
    read and unit codes present"""
    read, unit = rng.integers(0, n_reads, size=n), rng.integers(0, n_units, size=n)
    if n:
        read[0], unit[-1] = n_reads - 1, n_units - 1
    ties = np.array([0.0, -0.0, 0.25, 0.5, BELOW_ONE, TINY])
    tiebreak = np.where(rng.random(n) < 0.6, ties[rng.integers(0, len(ties), size=n)], rng.random(n))
    return _rows(read, unit, base + rng.integers(0, spread, size=n), tiebreak, n_reads, n_units, threshold)


def good_cases():
    """(name, case) pairs; a case is the keyword arguments of device_good_rows / host_good_rows"""
    rng = np.random.default_rng(401)
    out = [('no rows', _rows([], [], [], [], 3, 2, 0.9)), ('no rows, no reads', _rows([], [], [], [], 0, 0, None)),
           ('one row', _rows([2], [1], [-5], [0.5], 4, 2, 1.0))]
    for n, thr in ((300, 0.998), (1000, None), (3000, 0.995)):
        out.append((f'seeded {n}', _seeded(rng, n, n // 7 + 1, 6, thr)))
    for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        out.append((f'{n} rows', _seeded(rng, n, n // 7 + 1, 6, 0.996)))
        out.append((f'{n} rows of one group', _rows(np.zeros(n), np.zeros(n), np.full(n, 5), np.full(n, 0.5), 1, 1, 1.0)))
    # one read through 300 tiles on six units, scores from 100 adjacent values, 40 lower on unit 2 and 20 lower on unit 4: the bar
    # 0.95 * 599 = 569.05 leaves out unit 2 (at most 559) and keeps unit 4 (579)
    n = 300 * TILE
    unit = rng.integers(0, 6, size=n)
    out.append(('one read through 300 tiles', _rows(np.zeros(n), unit, 500 + rng.integers(0, 100, size=n) - 40 * (unit == 2) - 20 * (unit == 4),
                                                    rng.integers(0, 8, size=n) / 8, 1, 6, 0.95)))
    n = 5000
    out.append(('every read has one row', _rows(rng.permutation(n), rng.integers(0, 6, size=n), rng.integers(-9, 9, size=n), rng.random(n), n, 6, 1.0)))
    out.append(('one read', _seeded(rng, 700, 1, 6, 0.998)))
    for k in (255, 256, 257, 65536):
        out.append((f'{k} reads and {k} units', _seeded(rng, 3000, k, k, 0.997)))
    # score ties within a (read, unit) with equal and with unequal tiebreakers; every row of the input twice
    out.append(('ties', _rows([0] * 6 + [1] * 4, [3] * 6 + [0, 0, 1, 1], [5, 9, 9, 9, 2, 9] + [7, 7, 7, 7], [0.9, 0.4, 0.7, 0.1, 0.9, 0.7] + [0.5, 0.5, 0.0, -0.0], 2, 4, 1.0)))
    c = _seeded(rng, 900, 120, 6, 0.998)
    out.append(('every row twice', _rows(np.tile(c['read'], 2), np.tile(c['unit'], 2), np.tile(c['score'], 2), np.tile(c['tiebreak'], 2), 120, 6, 0.998)))
    out += threshold_edge_cases()
    return out


def threshold_edge_cases():
    """Each read has its best row on unit 0 and one more row on unit 1.  The bar is ONE float64 product:
    100 * 0.07 = 7.000000000000001 (a score of 7 is dropped, exact arithmetic would keep it), while 10 * 0.7 = 7.0 and
    100 * 0.9 = 90.0 round onto the integer (7 and 90 are kept, as pandas keeps them).  The case "best 10 at 70 %" was asked for
    with 7 dropped, on the premise that 10 * 0.7 is 7.000000000000001; in IEEE float64 it is exactly 7.0 (0.7 is just below 7/10 and
    the product rounds up onto 7), so the reference keeps the 7 and so does the case; "best 100 at 7 %" is the case that separates
    float64 from exact arithmetic."""
    def two(best, other, threshold):
        return _rows([0, 0], [0, 1], [best, other], [0.5, 0.5], 1, 2, threshold)
    return [('best 10 at 70 percent', two(10, 7, 0.7)), ('best 100 at 7 percent', two(100, 7, 0.07)), ('best 100 at 90 percent', two(100, 90, 0.9)), ('100 percent', two(503, 502, 1.0)),
            ('0 percent', two(503, -4, 0.0)), ('120 percent', two(503, 503, 1.2)), ('120 percent of a negative best', two(-10, -12, 1.2)),
            ('120 percent of 0', two(0, -1, 1.2)), ('no threshold', two(503, -4, None)),
            ('scores next to 2^53', two(2 ** 53 - 1, 2 ** 53 - 2, 1.0)), ('scores next to -2^53', two(-2 ** 53 + 2, -2 ** 53 + 1, BELOW_ONE))]


EDGE_RESULTS = {'best 10 at 70 percent': [0, 1], 'best 100 at 7 percent': [0], 'best 100 at 90 percent': [0, 1], '100 percent': [0], '0 percent': [0], '120 percent': [],
                '120 percent of a negative best': [0, 1], '120 percent of 0': [0], 'no threshold': [0, 1], 'scores next to 2^53': [0],
                'scores next to -2^53': []}   # (2^53 - 2) * (1 - 2^-53) rounds to 2^53 - 3: a negative best misses its own bar


def caller_shapes(case):
    """the case as its callers shape it: the units as assemblies, each unit split into three sequences, the single unit 0"""
    split = dict(case, unit=(case['unit'] * 3 + (np.arange(len(case['unit'])) * 7 // 3) % 3).astype(np.int32), n_units=case['n_units'] * 3)
    single = dict(case, unit=np.zeros(len(case['unit']), np.int32), n_units=1 if case['n_units'] else 0)
    return [('assemblies', case), ('sequences', split), ('single unit', single)]


# ---- cases for mpn_sum_by_key --------------------------------------------------------------------------------------------------
def _sums(key, n_keys, cols):
    return dict(key=np.asarray(key, np.int32), n_keys=int(n_keys), cols=[np.asarray(c, np.int64) for c in cols])


def sum_cases():
    """(name, case) pairs; a case is the keyword arguments of device_sum_by_key / host_sum_by_key"""
    rng = np.random.default_rng(402)

    def cols(n, n_cols, lo=-1000, hi=100000):
        return [rng.integers(lo, hi, size=n) for _ in range(n_cols)]
    out = [('no rows', _sums([], 3, [[], []])), ('no rows, no keys', _sums([], 0, [[]])), ('one row', _sums([1], 3, [[-5], [7]]))]
    for n_cols in range(1, 7):
        n = 500 + 400 * n_cols
        out.append((f'{n_cols} columns', _sums(rng.integers(0, 9, size=n), 12, cols(n, n_cols))))            # keys 9..11 have no rows
    for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        out.append((f'{n} rows', _sums(np.minimum(rng.integers(0, 40, size=n), 6), 7, cols(n, 6))))          # key 6 holds most rows
        out.append((f'{n} rows on one key', _sums(np.full(n, 2), 4, cols(n, 5))))
        out.append((f'{n} keys of one row', _sums(rng.permutation(n), n, cols(n, 6))))
    for k in (255, 256, 257, 65536):
        key = rng.integers(0, k, size=3000)
        key[0] = k - 1
        out.append((f'{k} keys', _sums(key, k, cols(3000, 3))))
    # 2^20 rows at the ends of the value domain: one key holds every +TOP (its sum is 2^20 * (2^32 - 1)), one every -TOP, one a mix
    n = 2 ** 20
    key = rng.integers(0, 3, size=n)
    out.append(('2^20 rows at the ends of the domain', _sums(key, 5, [np.where(key == 0, TOP, np.where(key == 1, -TOP, rng.choice([TOP, -TOP], size=n))),
                                                                   np.full(n, TOP), np.full(n, -TOP)])))
    return out


# ---- tables for the mirrors ----------------------------------------------------------------------------------------------------
TAX = pd.DataFrame({'assembly_id': ASSEMBLIES, 'tax_id': [11, 12, 21, 22, 31, 32], 'species_tax_id': [100, 100, 200, 200, 300, 300],
                    'genus_tax_id': [1000, 1000, 2000, 2000, 2000, 2000], 'genus_height': [2, 2, 2, 2, 3, 3]})
SPECIES_LIST = pd.DataFrame({'species_tax_id': [300, 100, 400, 200], 'species_name': ['c', 'a', 'absent', 'b']})   # 400 has no alignment
EQUAL_LENGTHS = pd.DataFrame({'assembly_id': ASSEMBLIES, 'assembly_length': [16000, 16000, 15500, 12000, 18000, 9000]})


def _with_species(table):
    species = dict(zip(TAX['assembly_id'], TAX['species_tax_id']))
    return table.assign(species_tax_id=[species[a] for a in table['assembly_id']])


def mirrored_table(seed):
    """The dedicated tie: the rows of A1 and a copy of each on A2 (its sequences renamed) with half the tiebreaker.  Under
    EQUAL_LENGTHS both assemblies of species 100 get the same sums, the same covered bp and so the same adjusted_average_depth; the
    summed tiebreakers, one half the other, decide the pick."""
    a1 = best_table(seed)
    a1 = a1[a1['assembly_id'] == 'A1']
    a2 = a1.assign(assembly_id='A2', sequence_id=a1['sequence_id'].str.replace('A1', 'A2'), alignment_score_tiebreaker=a1['alignment_score_tiebreaker'] * 0.5)
    a2.index = a1.index + 5000
    rest = best_table(seed + 1, n_reads=30)
    rest = rest[rest['assembly_id'].isin(['A3', 'A5'])]
    rest.index = rest.index + 20000
    both = pd.concat([a1, a2, rest])
    return both.iloc[np.random.default_rng(seed).permutation(len(both))]


def selection_cases():
    """name -> how the tables are made and the step's parameters.  min_depth lies between the species' picked depths wherever both
    counts should be non-zero."""
    return [dict(name='mixed', seed=171, threshold=99.8, min_depth=4.0, noise_seed=None),
            dict(name='mixed, sequences under a noise BED', seed=172, threshold=99.6, min_depth=5.0, noise_seed=5),
            dict(name='wide scores', seed=173, n_reads=40, spread=40, threshold=95, min_depth=3.0, noise_seed=6),
            dict(name='every row tied', seed=174, n_reads=25, all_tied=True, threshold=100, min_depth=1.0, noise_seed=None),
            dict(name='few rows', seed=175, n_reads=30, rows_per_read=1, spread=1, threshold=70, min_depth=0.5, noise_seed=None),
            dict(name='two assemblies of equal depth', seed=176, mirrored=True, threshold=99.8, min_depth=1.0, noise_seed=None)]


def selection_inputs(case):
    """-> dict(species_align_list, assembly_align_list, species_list, read_id_species_id, assembly_length, assembly_tax,
    sequence_length, noise_bed).  The index labels of the two tables do not overlap."""
    kw = {k: case[k] for k in ('n_reads', 'rows_per_read', 'all_tied', 'spread') if k in case}
    species = _with_species(mirrored_table(case['seed']) if case.get('mirrored') else best_table(case['seed'], **kw))
    assembly = _with_species(best_table(case['seed'] + 1000, **dict(kw, n_reads=max(10, kw.get('n_reads', 60) // 2))))
    assembly.index = assembly.index + 100000
    rng = np.random.default_rng(case['seed'])
    reads = sorted(set(species['read_id']))
    first = species.drop_duplicates('read_id').set_index('read_id')['species_tax_id']
    placed = pd.DataFrame({'read_id': reads, 'species_tax_id': [int(first[r]) if rng.random() < 0.8 else 100 for r in reads]})
    placed = placed[rng.random(len(placed)) < 0.9]                              # a tenth of the reads was placed nowhere
    seqs = sorted(set(species['sequence_id']) | set(assembly['sequence_id']))
    return dict(species_align_list=species, assembly_align_list=assembly, species_list=SPECIES_LIST, read_id_species_id=placed,
                assembly_length=EQUAL_LENGTHS if case.get('mirrored') else LENGTHS, assembly_tax=TAX,
                sequence_length=pd.DataFrame({'sequence_id': seqs, 'sequence_length': [8000 if s.endswith('c1') else 7500 for s in seqs]}),
                noise_bed=noise_bed_for(species, case['noise_seed']) if case['noise_seed'] is not None else None)


def inputs_digest(inp):
    return [table_digest(inp['species_align_list']), table_digest(inp['assembly_align_list'])]


# ---- frames as golden records --------------------------------------------------------------------------------------------------
def frame_record(frame, values=True):
    """index labels in order, columns; with `values` the integer columns as ints, the float columns as float.hex(), the others as str"""
    rec = dict(index=[int(i) for i in frame.index], columns=[str(c) for c in frame.columns])
    if values:
        rec['int'] = {c: [int(v) for v in frame[c]] for c in frame.columns if pd.api.types.is_integer_dtype(frame[c])}
        rec['float'] = {c: [float(v).hex() for v in frame[c]] for c in frame.columns if pd.api.types.is_float_dtype(frame[c])}
        rec['str'] = {c: [str(v) for v in frame[c]] for c in frame.columns if c not in rec['int'] and c not in rec['float']}
    return rec


def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'assembly_selection_golden.json')) as f:
        return json.load(f)['cases']


SUMMED_FLOAT = 'alignment_score_tiebreaker'   # the one float SUM: pandas adds with compensation, np.bincount without


def check_frame(frame, rec, name, rows_summed=None, source=None):
    """frame against its golden record.  Index order, columns, integer and string columns: exactly.  Float columns: bit for bit,
    but the summed tiebreaker within n * 2^-52 relative, n = rows_summed[i] rows in the sum (all terms are >= 0, so that bounds
    what an order or a compensation of the additions can change).  source: for a frame stored without values, the table whose rows
    under the same labels it must equal."""
    assert [int(i) for i in frame.index] == rec['index'] and [str(c) for c in frame.columns] == rec['columns'], name
    if 'int' not in rec:
        assert frame.equals(source.loc[rec['index']][rec['columns']]), name
        return
    for c, want in rec['int'].items():
        assert pd.api.types.is_integer_dtype(frame[c]) and [int(v) for v in frame[c]] == want, (name, c)
    for c, want in rec['str'].items():
        assert [str(v) for v in frame[c]] == want, (name, c)
    for c, want in rec['float'].items():
        assert frame[c].dtype == np.float64, (name, c)
        if c == SUMMED_FLOAT and rows_summed is not None:
            for got, w, n in zip(frame[c], want, rows_summed):
                w = float.fromhex(w)
                assert abs(float(got) - w) <= int(n) * 2.0 ** -52 * abs(w), (name, c, got, w)
        else:
            assert [float(v).hex() for v in frame[c]] == want, (name, c)
