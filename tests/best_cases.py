"""Cases and brute-force statements shared by tests/test_best_align.py (CPU), tests/test_best_align_gpu.py and
tests/golden/make_best_align_golden.py: the candidates of a read for its best alignment, the abundance-weighted draw among them and
the second best score, in plain loops over dicts."""
import hashlib
import json
import math
import os
import random

import numpy as np
import pandas as pd

BELOW_ONE = math.nextafter(1.0, 0.0)
TINY = 5e-324                                                      # the smallest denormal
COLUMNS = ['read_id', 'read_length', 'assembly_id', 'sequence_id', 'sequence_length', 'sequence_from', 'sequence_to', 'match', 'edit_dist',
           'alignment_score', 'alignment_score_tiebreaker']


# ---- brute force ---------------------------------------------------------------------------------------------------------------
def brute_candidates(read, assembly, score, tiebreak, n_reads):
    """-> cand_row, cand_read, read_count, read_first as lists"""
    kept = {}
    for i in range(len(read)):
        key = (int(read[i]), int(assembly[i]))
        j = kept.get(key)
        if j is None or (int(score[i]), float(tiebreak[i])) >= (int(score[j]), float(tiebreak[j])):   # a later equal row replaces
            kept[key] = i
    best = {}
    for (r, _), i in kept.items():
        best[r] = max(best.get(r, int(score[i])), int(score[i]))
    cand_row, cand_read, count = [], [], [0] * n_reads
    for (r, a) in sorted(kept):
        i = kept[(r, a)]
        if int(score[i]) == best[r]:
            cand_row.append(i)
            cand_read.append(r)
            count[r] += 1
    first, at = [], 0
    for c in count:
        first.append(at)
        at += c
    return cand_row, cand_read, count, first


def brute_pick(read, weight, tiebreak, draw, n_reads):
    """-> new_tiebreak (floats), winner as lists"""
    members = {}
    for j in range(len(read)):
        members.setdefault(int(read[j]), []).append(j)
    new, winner = [0.0] * len(read), [-1] * n_reads
    for r, js in members.items():
        total = sum(int(weight[j]) for j in js)
        for j in js:
            if len(js) == 1:
                new[j] = float(tiebreak[j])
            else:
                new[j] = float(draw[j]) * (1.0 if total <= 0 else float(int(weight[j])) / float(total))
        top = js[0]
        for j in js[1:]:
            if new[j] >= new[top]:
                top = j
        winner[r] = top
    return new, winner


def brute_second(read, assembly, score, n_reads, excluded):
    out = [None] * n_reads
    for i in range(len(read)):
        r = int(read[i])
        if int(assembly[i]) != int(excluded[r]) and (out[r] is None or int(score[i]) > out[r]):
            out[r] = int(score[i])
    return [0 if v is None else v for v in out]


def brute_best_align_list(table, abundance_of, rng):
    """table: DataFrame.  abundance_of(labels of the one-candidate reads' rows) -> {assembly_id: abundance}.  -> the index labels of
    the winning rows in read_id order, their new tiebreakers, the number of draws"""
    rows = [dict(label=label, **rec) for label, rec in zip(table.index, table.to_dict('records'))]
    kept = {}
    for row in rows:
        key = (str(row['read_id']), str(row['assembly_id']))
        old = kept.get(key)
        if old is None or (row['alignment_score'], row['alignment_score_tiebreaker']) >= (old['alignment_score'], old['alignment_score_tiebreaker']):
            kept[key] = row
    by_read = {}
    for key in sorted(kept):
        by_read.setdefault(key[0], []).append(kept[key])
    cands = {r: [x for x in rs if x['alignment_score'] == max(y['alignment_score'] for y in rs)] for r, rs in by_read.items()}
    alone = [c[0]['label'] for c in cands.values() if len(c) == 1]
    several = any(len(c) > 1 for c in cands.values())
    abundance = abundance_of(alone) if alone and several else {}
    labels, tiebreakers, draws = [], [], 0
    for r in sorted(cands):
        c = cands[r]
        if len(c) == 1:
            labels.append(c[0]['label'])
            tiebreakers.append(float(c[0]['alignment_score_tiebreaker']))
            continue
        total = sum(int(abundance.get(str(x['assembly_id']), 0)) for x in c)
        top = None
        for x in c:
            draws += 1
            w = int(abundance.get(str(x['assembly_id']), 0))
            t = rng() * (1.0 if total <= 0 else float(w) / float(total))
            if top is None or t >= top[0]:
                top = (t, x['label'])
        labels.append(top[1])
        tiebreakers.append(top[0])
    return labels, tiebreakers, draws


def read_classes(table):
    """-> reads with one candidate, reads with several, assemblies without a one-candidate read (plain loops)"""
    n_cand, kept = {}, {}
    for rec in table.to_dict('records'):
        key = (rec['read_id'], rec['assembly_id'])
        kept[key] = max(kept.get(key, rec['alignment_score']), rec['alignment_score'])
    top = {}
    for (r, _), s in kept.items():
        top[r] = max(top.get(r, s), s)
    alone_asm = set()
    for (r, a), s in kept.items():
        if s == top[r]:
            n_cand[r] = n_cand.get(r, 0) + 1
    for (r, a), s in kept.items():
        if s == top[r] and n_cand[r] == 1:
            alone_asm.add(a)
    one = sum(1 for v in n_cand.values() if v == 1)
    return one, len(n_cand) - one, sorted(set(table['assembly_id']) - alone_asm)


# ---- cases for the entries ---------------------------------------------------------------------------------------------------
def random_small_case(rng):
    """1-6 reads, 1-6 assemblies, 0-40 rows; scores from four adjacent values around a base that may be negative or huge;
    tiebreakers from a handful of values (so that whole rows tie) or random."""
    n_reads, n_asm, n = int(rng.integers(1, 7)), int(rng.integers(1, 7)), int(rng.integers(0, 41))
    base = int(rng.choice([0, -2, 100, -(2 ** 63) + 1, 2 ** 63 - 4]))
    score = (base + rng.integers(0, 4, size=n)).astype(np.int64) if n else np.zeros(0, np.int64)
    ties = np.array([0.0, -0.0, 0.25, 0.5, BELOW_ONE, TINY, 2 * TINY])
    tiebreak = np.where(rng.random(n) < 0.6, ties[rng.integers(0, len(ties), size=n)], rng.random(n))
    return dict(read=rng.integers(0, n_reads, size=n).astype(np.int32), assembly=rng.integers(0, n_asm, size=n).astype(np.int32), score=score,
                tiebreak=tiebreak, n_reads=n_reads, n_assemblies=n_asm)


def random_pick_case(rng, cand_read, n_reads):
    """weights and draws for a candidate list: reads whose weights are all 0, one 0 among positive ones, sums near 2^52, equal draws"""
    m = len(cand_read)
    kind = rng.integers(0, 4, size=n_reads)[cand_read] if m else np.zeros(0, np.int64)
    weight = np.where(kind == 0, 0, np.where(kind == 1, rng.integers(0, 3, size=m), np.where(kind == 2, rng.integers(0, 2 ** 49, size=m), rng.integers(0, 1000, size=m))))
    draws = np.array([0.0, 0.5, BELOW_ONE, TINY, 0.75])
    draw = np.where(rng.random(m) < 0.5, draws[rng.integers(0, len(draws), size=m)], rng.random(m))
    tiebreak = rng.random(m)
    return dict(read=np.asarray(cand_read, dtype=np.int32), weight=weight.astype(np.int64), tiebreak=tiebreak, draw=draw, n_reads=n_reads)


# ---- tables for the mirrors --------------------------------------------------------------------------------------------------
ASSEMBLIES = ['A1', 'A2', 'A3', 'A4', 'A5', 'A6']
LENGTHS = pd.DataFrame({'assembly_id': ASSEMBLIES, 'assembly_length': [16000, 17000, 15500, 12000, 18000, 9000]})


def best_table(seed, n_reads=60, rows_per_read=7, all_tied=False, spread=4):
    """A seeded alignment table in shuffled row order under shuffled index labels: about rows_per_read rows per read on A1..A5 with
    scores from `spread` adjacent values and tiebreakers that repeat, and now and then a row on A6 that copies the score of another
    row of its read -- so A6 is a candidate only together with another assembly and never has a read of its own.
    all_tied: every row has one score and one tiebreaker."""
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(n_reads):
        mine = []
        for _ in range(int(rng.integers(max(1, rows_per_read - 3), rows_per_read + 4))):
            a = ASSEMBLIES[int(rng.integers(0, 5))]
            mine.append((a, 500 if all_tied else 500 + int(rng.integers(0, spread)), 0.5 if all_tied else float(rng.choice([0.25, 0.5, rng.random()]))))
        if rng.random() < 0.35:
            mine.append(('A6', mine[int(rng.integers(0, len(mine)))][1], 0.5 if all_tied else float(rng.random())))
        for a, s, t in mine:
            seq = a + ('_c1' if rng.random() < 0.7 else '_c2')
            s0 = int(rng.integers(0, 4000))
            e0 = s0 + int(rng.integers(50, 3000))
            rows.append((f'r{r:03d}' if r % 7 else f'R{r}', 5000, a, seq, 8000, s0, e0, max(1, (e0 - s0) // 2), 5, s, t))
    order = rng.permutation(len(rows))
    table = pd.DataFrame([rows[i] for i in order], columns=COLUMNS)
    table.index = 1000 + rng.permutation(len(rows))
    return table


def noise_bed_for(table, seed):
    rng = np.random.default_rng(seed)
    pairs = table[['assembly_id', 'sequence_id']].drop_duplicates().sort_values(['assembly_id', 'sequence_id'])
    rows = []
    for a, s in zip(pairs['assembly_id'], pairs['sequence_id']):
        for _ in range(2):
            s0 = int(rng.integers(0, 6000))
            rows.append((s, s0, s0 + int(rng.integers(100, 1500)), a))
    return pd.DataFrame(rows, columns=['sequence_id', 'start', 'end', 'assembly_id'])


def other_best_table(table, seed, prefix):
    """a human / decoy best table: one row for about a third of the reads, scores around the table's"""
    rng = np.random.default_rng(seed)
    reads = sorted(set(table['read_id']))
    picked = [r for r in reads if rng.random() < 0.33] + [prefix + '_only']
    return pd.DataFrame({'read_id': picked, 'assembly_id': [prefix] * len(picked), 'alignment_score': [int(rng.integers(495, 505)) for _ in picked],
                         'alignment_score_tiebreaker': [float(rng.random()) for _ in picked]})


def golden_cases():
    """name -> arguments of best_table, and whether a noise BED goes in"""
    return [dict(name='mixed', table=dict(seed=71)), dict(name='mixed with a noise BED', table=dict(seed=72), noise_seed=5),
            dict(name='every row tied', table=dict(seed=73, n_reads=25, all_tied=True)),
            dict(name='wide scores', table=dict(seed=74, n_reads=40, spread=40)),
            dict(name='few rows, one score', table=dict(seed=75, n_reads=30, rows_per_read=1, spread=1)),
            dict(name='long', table=dict(seed=76, n_reads=150, rows_per_read=5))]


def table_digest(table):
    return hashlib.sha1(json.dumps(dict(index=[int(i) for i in table.index], rows=table.to_dict('list')), sort_keys=True).encode()).hexdigest()


def counter_rng():
    """rng() = k / 2^20 at its k-th call (k from 1); .calls: how many"""
    def rng():
        rng.calls += 1
        return rng.calls / 2 ** 20
    rng.calls = 0
    return rng


# ---- the mirrors against the goldens and the brute force ------------------------------------------------------------------------
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'best_align_golden.json')) as f:
        return json.load(f)['cases']


def golden_inputs(rec):
    table = best_table(**rec['table'])
    assert table_digest(table) == rec['table_sha1'], 'the seeded table is not the one the golden was made from'
    return table, (noise_bed_for(table, rec['noise_seed']) if rec['noise_seed'] is not None else None)


def check_against_golden(rec, device):
    """the four mirrors on one golden case: index labels, their order, columns, tiebreakers bit for bit, the position of the global
    random stream afterwards"""
    from megapath_nano_amd import abundance
    table, noise = golden_inputs(rec)
    random.seed(rec['seed'])
    best = abundance.align_list_to_best_align_list(align_list=table, assembly_length=LENGTHS, noise_bed=noise, device=device)
    assert random.random().hex() == rec['next_random'], rec['name']
    assert list(best.columns) == rec['columns'] and [int(i) for i in best.index] == rec['index'], rec['name']
    assert [float(x).hex() for x in best['alignment_score_tiebreaker']] == rec['tiebreaker'], rec['name']
    assert best.drop(columns='alignment_score_tiebreaker').equals(table.loc[rec['index']].drop(columns='alignment_score_tiebreaker')), rec['name']

    want = rec['short_alignment_removal']
    random.seed(rec['seed'])
    out, before, after = abundance.short_alignment_removal(align_list=table, min_align_length=want['min_align_length'], assembly_length=LENGTHS, device=device)
    assert ([int(i) for i in out.index], list(out.columns), before, after) == (want['index'], want['columns'], want['num_read_before'], want['num_read_after']), rec['name']
    assert out.equals(table.loc[want['index']]), rec['name']

    want = rec['unique_alignment']
    human, decoy = other_best_table(table, want['human_seed'], 'human'), other_best_table(table, want['decoy_seed'], 'decoy')
    out, before, after = abundance.unique_alignment(align_list=table, best_align_list=best, human_best_align_list=human, decoy_best_align_list=decoy,
                                                    unique_align_threshold=want['unique_align_threshold'], device=device)
    assert ([int(i) for i in out.index], list(out.columns), before, after) == (want['index'], want['columns'], want['num_read_before'], want['num_read_after']), rec['name']
    assert [int(x) for x in out['second_best_alignment_score']] == want['second_best'] and out['second_best_alignment_score'].dtype == np.int64, rec['name']
    return best


def check_against_brute_force(table, noise, device):
    """align_list_to_best_align_list under a counting rng against the loops; -> the number of draws"""
    from megapath_nano_amd import abundance

    def abundance_of(labels):
        stat = abundance.align_stat_by_assembly_id(table.loc[labels], LENGTHS, None, noise_bed=noise, device=False)
        return dict(zip(stat['assembly_id'], stat['adjusted_total_aligned_bp']))
    rng, loop_rng = counter_rng(), counter_rng()
    best = abundance.align_list_to_best_align_list(align_list=table, assembly_length=LENGTHS, noise_bed=noise, rng=rng, device=device)
    labels, tiebreakers, draws = brute_best_align_list(table, abundance_of, loop_rng)
    assert list(best.index) == labels and rng.calls == draws == loop_rng.calls
    assert [float(x).hex() for x in best['alignment_score_tiebreaker']] == [t.hex() for t in tiebreakers]
    assert list(best['read_id']) == sorted(set(table['read_id']))
    return draws
