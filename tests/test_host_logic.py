"""CPU tests (no GPU): host-side logic of the mirrors -- minimap2 argv parsing, FASTA/FASTQ readers, species-name
rule, shard balancing -- and the N>1 plumbing with world_size-2 gloo processes."""
import gzip
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_species_name_rule_matches_reference_lambda():
    from megapath_nano_amd.reassignment import species_name
    ref = lambda x: " ".join(x.split(" ", 2)[0:2]) if ' sp. ' not in x else " ".join(x.split(" ", 3)[0:3])  # noqa: E731
    for d in ['Escherichia coli strain K-12 substr. MG1655, complete genome', 'Bacillus sp. X1(2014) chromosome', 'Plasmid',
              'A b', 'Candidatus Pelagibacter sp. HTCC7211 x', '']:
        assert species_name(d, 'species') == ref(d)
        assert species_name(d, 'strain') == d


def test_parse_aligner_options(libmpn):
    from megapath_nano_amd.aligner import parse_aligner_options
    opt, k, w = parse_aligner_options(['-t', '64', '-I', '0G', '-N', '50', '-p', '1', '-x', 'map-ont', '--split-prefix', 'tmp'], False)
    assert (opt.best_n, opt.pri_ratio, opt.with_cigar, k, w) == (50, 1.0, 1, 15, 10)
    opt, k, w = parse_aligner_options(['-t8', '-x', 'map-ont'], True)
    assert (opt.best_n, round(opt.pri_ratio, 3), opt.with_cigar) == (5, 0.8, 0)
    opt, k, w = parse_aligner_options(['-k15', '-w15', '-A1', '-B4', '-O1', '-E2', '-s50', '-z50', '-N', '1000', '-p', '0'], False)
    assert (k, w, opt.a, opt.b, opt.q, opt.e, opt.min_dp_max, opt.zdrop, opt.best_n, opt.pri_ratio) == (15, 15, 1, 4, 1, 2, 50, 50, 1000, 0.0)
    with pytest.raises(ValueError):
        parse_aligner_options(['-x', 'sr'], False)


def test_read_fastx(tmp_path):
    from megapath_nano_amd.aligner import read_fastx
    fa = tmp_path / 'a.fna.gz'
    with gzip.open(fa, 'wb') as f:
        f.write(b'>s1 desc\nACGT\nAC\n>s2\nTTTT\n')
    with gzip.open(fa, 'ab') as f:  # concatenated gzip members, as `cat *.fna.gz` into the FIFO (aligner.py:209-217)
        f.write(b'>s3\nGG\n')
    assert read_fastx(str(fa)) == [('s1', b'ACGTAC'), ('s2', b'TTTT'), ('s3', b'GG')]
    fq = tmp_path / 'r.fq'
    fq.write_bytes(b'@r1 x\nACGT\n+\nIIII\n@r2\nAC\nGT\n+r2\n@@\n@I\n')
    assert read_fastx(str(fq)) == [('r1', b'ACGT'), ('r2', b'ACGT')]


def test_shard_bounds_balance_bases():
    from megapath_nano_amd.dist import shard_bounds
    rng = np.random.default_rng(0)
    lens = rng.integers(200, 50000, size=1000)
    for world in (1, 2, 3, 8):
        b = shard_bounds(lens, world)
        assert b[0][0] == 0 and b[-1][1] == len(lens) and all(b[i][1] == b[i + 1][0] for i in range(world - 1))
        sums = [int(lens[lo:hi].sum()) for lo, hi in b]
        assert max(sums) - min(sums) <= 2 * int(lens.max())
    assert shard_bounds([], 4) == [(0, 0)] * 4


GLOO_WORKER = textwrap.dedent('''
    import os, sys, json
    import numpy as np
    sys.path.insert(0, %r)
    from megapath_nano_amd import dist as mdist
    rank, world, local = mdist.init_from_env(backend='gloo')
    ar = mdist.make_allreduce(None)
    # two-shard decomposition of the counters around the reassignment pass: the oracle stands in for the HIP
    # kernels here (CPU test of the orchestration only)
    sys.path.insert(0, os.path.join(%r, 'tests'))
    from reassign_cases import community, SPECIES
    from oracle import reassign_oracle as ro
    table = community(5, 600, [50, 0, 2, 1, 30, 0, 0, 0, 0, 0, 0, 0], {0: [(2, 0.5), (3, 0.3)], 2: [(0, 0.9)], 3: [(0, 0.9)]})
    reads = sorted(set(table['read_id']))
    lo, hi = mdist.shard_bounds([1] * len(reads), world)[rank]
    mine = set(reads[lo:hi])
    keep = [i for i, r in enumerate(table['read_id']) if r in mine]
    part = {k: [v[i] for i in keep] for k, v in table.items()}
    res = ro.reassign_oracle(part, SPECIES)
    names = sorted({ro.species_name(d, 'species') for _, d in SPECIES})
    code = {n: i for i, n in enumerate(names)}
    local_counts = np.zeros(len(names), dtype=np.int64)
    for n, c in ro.read_count_by_name(part, res['rows']).items():
        local_counts[code[n]] += c
    total = local_counts.copy()
    ar(total)
    # tiebreakers in global row order: every rank seeds the same stream, rank r owns 100 + 37 * r rows, two steps
    import random
    from megapath_nano_amd.pipeline import sharded_tiebreak
    rnd = random.Random('reads.fq')
    tb = [sharded_tiebreak(rnd, 100 + 37 * rank, (rank, world), ar).tolist() for _ in range(2)]
    mdist.barrier()
    with open(os.path.join(os.environ['MPN_TEST_OUT'], f'rank{rank}.json'), 'w') as f:
        json.dump(dict(rank=rank, local=int(local_counts.sum()), total=[int(x) for x in total], n_reads=len(reads), tb=tb,
                       next=rnd.random()), f)
''')


def test_gloo_world2_count_allreduce(tmp_path, oracle_built):
    script = tmp_path / 'worker.py'
    script.write_text(GLOO_WORKER % (ROOT, ROOT))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MPN_TEST_OUT=str(tmp_path))
    out = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
                          '--master-addr', '127.0.0.1', '--master-port', '29533', str(script)],
                         capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    import json
    lines = [json.load(open(tmp_path / f'rank{r}.json')) for r in range(2)]
    assert sorted(l['rank'] for l in lines) == [0, 1]
    assert lines[0]['total'] == lines[1]['total']
    assert sum(lines[0]['total']) == lines[0]['n_reads'] == lines[0]['local'] + lines[1]['local']
    # the two ranks' tiebreakers, concatenated in rank order, are one random.random() stream (aligner.py:334-335)
    import random
    lines.sort(key=lambda l: l['rank'])
    want = random.Random('reads.fq')
    for step in range(2):
        for l in lines:
            assert l['tb'][step] == [want.random() for _ in range(len(l['tb'][step]))]
    nxt = want.random()
    assert lines[0]['next'] == lines[1]['next'] == nxt


def test_random_block_is_the_python_stream():
    import random
    from megapath_nano_amd.pipeline import random_block, sharded_tiebreak
    import hashlib
    seed = hashlib.md5('reads.fq'.encode()).hexdigest()                     # aligner.py:167-168
    a, b = random.Random(seed), random.Random(seed)
    assert random_block(a, 3).tolist() == [0.2507641374631844, 0.3100258391581491, 0.8083515623068414]
    b.random(), b.random(), b.random()
    for n in (0, 1, 623, 624, 625, 5000):
        assert random_block(a, n).tolist() == [b.random() for _ in range(n)]
    assert a.random() == b.random()
    assert sharded_tiebreak(a, 7, (0, 1), None).tolist() == [b.random() for _ in range(7)]


def test_human_decoy_classification_rules():
    """megapath_nano.py:1135-1200 on a hand-made table: human first, then decoy on the rest, microbe = remainder."""
    import pandas as pd
    from megapath_nano_amd.filters import human_and_decoy_classify
    rows = [
        # read, len, assembly, AS, tiebreak
        ('h_abs', 5000, 'HUMAN', 1200, .1),      # AS >= 1000
        ('h_pct', 600, 'HUMAN', 650, .2),        # AS*100/len >= 100
        ('h_low', 5000, 'HUMAN', 300, .3),       # below both thresholds: not human
        ('h_low', 5000, 'DECOY', 1500, .4),      # ... but decoy
        ('both', 3000, 'HUMAN', 2000, .5), ('both', 3000, 'DECOY', 2500, .6),   # human wins (filtered first)
        ('m1', 4000, 'MIC1', 3000, .7), ('m1', 4000, 'MIC2', 3000, .8),         # tie -> tiebreaker picks MIC2
        ('m2', 4000, 'MIC1', 900, .9), ('m2', 4000, 'DECOY', 100, .05),         # weak decoy hit stays microbe
    ]
    al = pd.DataFrame(rows, columns=['read_id', 'read_length', 'assembly_id', 'alignment_score', 'alignment_score_tiebreaker'])
    reads = pd.DataFrame({'read_id': ['h_abs', 'h_pct', 'h_low', 'both', 'm1', 'm2', 'unaligned'],
                          'read_length': [5000, 600, 5000, 3000, 4000, 4000, 777]})
    out = human_and_decoy_classify(al, pd.DataFrame({'assembly_id': ['HUMAN']}), pd.DataFrame({'assembly_id': ['DECOY']}), reads)
    assert sorted(out['human_read_id_list']['read_id']) == ['both', 'h_abs', 'h_pct']
    assert sorted(out['decoy_read_id_list']['read_id']) == ['h_low']
    assert sorted(out['microbe_read_id_list']['read_id']) == ['m1', 'm2', 'unaligned']
    mb = out['microbe_best_align_list'].set_index('read_id')
    assert mb.loc['m1', 'assembly_id'] == 'MIC2' and mb.loc['m2', 'assembly_id'] == 'MIC1'


def test_human_decoy_classification_randomised_against_plain_loops():
    """The integer-coded classification against a dictionary-and-loops restatement of the same rules, on random tables with
    score ties, reads hitting several sets, reads without alignments."""
    import pandas as pd
    from megapath_nano_amd.filters import human_and_decoy_classify
    rng = np.random.default_rng(5)
    for trial in range(20):
        n_reads = int(rng.integers(1, 60))
        lens = {f'r{i:03d}': int(rng.integers(200, 6000)) for i in range(n_reads)}
        rows = []
        for rid, L in lens.items():
            for _ in range(int(rng.integers(0, 5))):
                rows.append((rid, L, str(rng.choice(['H1', 'H2', 'D1', 'M1', 'M2', 'M3'])), int(rng.choice([50, 500, 999, 1000, 1001, L, L - 1, 3000])),
                             float(rng.random())))
        al = pd.DataFrame(rows, columns=['read_id', 'read_length', 'assembly_id', 'alignment_score', 'alignment_score_tiebreaker'])
        reads = pd.DataFrame({'read_id': list(lens), 'read_length': list(lens.values())})
        out = human_and_decoy_classify(al, pd.DataFrame({'assembly_id': ['H1', 'H2']}), pd.DataFrame({'assembly_id': ['D1']}), reads)
        # plain restatement
        def best(rows_):
            b = {}
            for r in rows_:
                if r[0] not in b or (r[3], r[4]) > (b[r[0]][3], b[r[0]][4]):
                    b[r[0]] = r
            return b
        ok = lambda r: r[3] >= 1000 or r[3] * 100 / r[1] >= 100  # noqa: E731
        human = {k for k, r in best([r for r in rows if r[2] in ('H1', 'H2')]).items() if ok(r)}
        rest = [r for r in rows if r[0] not in human]
        decoy = {k for k, r in best([r for r in rest if r[2] == 'D1']).items() if ok(r)}
        micro = best([r for r in rest if r[0] not in decoy])
        assert set(out['human_read_id_list']['read_id']) == human and set(out['decoy_read_id_list']['read_id']) == decoy
        assert set(out['microbe_read_id_list']['read_id']) == set(lens) - human - decoy
        got = {t.read_id: (t.assembly_id, t.alignment_score, t.alignment_score_tiebreaker) for t in out['microbe_best_align_list'].itertuples()}
        assert got == {k: (r[2], r[3], r[4]) for k, r in micro.items()}
        assert list(out['microbe_best_align_list']['read_id']) == sorted(micro)


def test_abundance_statistic_against_plain_restatement():
    """align_stat_by_assembly_id (megapath_nano.py:485-541, default configuration) on random tables: best row per
    (read, assembly), sums, interval-union coverage with book-ended intervals merged, derived columns."""
    import pandas as pd
    from megapath_nano_amd.abundance import align_stat_by_assembly_id, covered_bp_by_assembly
    t = pd.DataFrame({'assembly_id': ['A'] * 5 + ['B'] * 2, 'sequence_id': ['s1', 's1', 's1', 's2', 's1', 's1', 's1'],
                      'sequence_from': [0, 10, 20, 0, 100, 5, 5], 'sequence_to': [10, 20, 25, 7, 130, 9, 9]})
    assert covered_bp_by_assembly(t, device=False) == {'A': 25 + 7 + 30, 'B': 4}
    noise = pd.DataFrame({'sequence_id': ['s1', 's1', 's9'], 'start': [5, 110, 0], 'end': [12, 200, 50], 'assembly_id': ['A', 'A', 'Z']})
    assert covered_bp_by_assembly(t, noise_bed=noise, device=False) == {'A': (25 - 7) + 7 + (30 - 20), 'B': 4 - 4}
    rng = np.random.default_rng(11)
    for trial in range(10):
        rows = []
        for r in range(int(rng.integers(1, 80))):
            L = int(rng.integers(500, 9000))
            for _ in range(int(rng.integers(1, 4))):
                a = str(rng.choice(['A1', 'A2', 'A3']))
                s0 = int(rng.integers(0, 3000))
                e0 = s0 + int(rng.integers(1, 2500))
                rows.append((f'r{r}', L, a, a + str(rng.choice(['_c1', '_c2'])), s0, e0, int(rng.integers(1, e0 - s0 + 1)), int(rng.integers(0, 200)),
                             int(rng.choice([100, 200, 200, 900])), float(rng.random())))
        al = pd.DataFrame(rows, columns=['read_id', 'read_length', 'assembly_id', 'sequence_id', 'sequence_from', 'sequence_to', 'match',
                                         'edit_dist', 'alignment_score', 'alignment_score_tiebreaker'])
        lens = pd.DataFrame({'assembly_id': ['A1', 'A2'], 'assembly_length': [4000, 0]})   # A3 unknown, A2 zero length
        got = align_stat_by_assembly_id(al, lens, device=False).set_index('assembly_id')
        best = {}
        for row in rows:
            key = (row[0], row[2])
            if key not in best or (row[8], row[9]) > (best[key][8], best[key][9]):
                best[key] = row
        for a in sorted({k[1] for k in best}):
            mine = [v for k, v in best.items() if k[1] == a]
            covered = set()
            for v in mine:
                covered |= {(v[3], p) for p in range(v[4], v[5])}
            L = {'A1': 4000, 'A2': 0}.get(a, 0)
            tab = sum(v[5] - v[4] for v in mine)
            g = got.loc[a]
            assert (g['total_number_of_read'], g['total_read_bp'], g['total_aligned_bp'], g['match'], g['covered_bp']) == \
                   (len(mine), sum(v[1] for v in mine), tab, sum(v[6] for v in mine), len(covered))
            if L:
                acp = len(covered) / L
                assert abs(g['adjusted_average_depth'] - acp * tab / L) < 1e-12 and g['adjusted_total_aligned_bp'] == int(round(acp * tab / L * L))
                assert abs(g['average_identity'] - sum(v[6] for v in mine) / tab) < 1e-12
            else:
                assert g['average_depth'] == 0 and g['adjusted_average_depth'] == 0 and g['adjusted_total_aligned_bp'] == 0


def test_index_file_magic_detection(tmp_path):
    """`Align()` / bin/mpn-aligner treat a target as a saved index only if it carries the magic (no GPU needed to tell)."""
    from megapath_nano_amd.mapper import Index
    fa = tmp_path / 't.fa'
    fa.write_bytes(b'>s\nACGT\n')
    idx = tmp_path / 't.mpi'
    idx.write_bytes(Index.MAGIC + b'\0' * 64)
    assert not Index.is_index_file(str(fa)) and Index.is_index_file(str(idx)) and not Index.is_index_file(str(tmp_path / 'missing'))


def test_paf_check_numpy_walk_equals_the_plain_walk():
    """bench.py's correctness block uses paf_check.walk_np; it must give what the per-base loop gives."""
    import paf_check as pc
    rng = np.random.default_rng(11)
    sc = pc.Scoring()
    for _ in range(200):
        n = int(rng.integers(1, 40))
        cig = [(int(rng.integers(1, 30 if k % 2 == 0 else 60)), 'M' if k % 2 == 0 else 'ID'[int(rng.integers(0, 2))]) for k in range(n)]
        ql, tl = sum(l for l, o in cig if o != 'D'), sum(l for l, o in cig if o != 'I')
        q = ''.join(rng.choice(list('ACGTN'), p=[.24, .24, .24, .24, .04], size=ql))
        t = ''.join(rng.choice(list('ACGTN'), p=[.24, .24, .24, .24, .04], size=tl))
        assert pc.walk(cig, q, t, sc) == pc.walk_np(cig, q, t, sc)
    with pytest.raises(AssertionError):
        pc.walk_np([(3, 'M')], 'ACG', 'ACGT', sc)


def test_bench_refuses_more_ranks_than_gpus():
    """`bench.py --gpus N` without a launcher starts N ranks itself or exits non-zero: never a silent one-rank run
    (VERDICT r2).  Here no GPU is visible, so --gpus 2 must fail before anything is launched."""
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MPN_SINGLE_DEVICE')}
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '1', '--warmup', '0'],
                         capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode != 0 and 'GPU(s) are visible' in out.stderr and not out.stdout.strip()
    env['WORLD_SIZE'] = '4'
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2'], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode != 0 and 'WORLD_SIZE=4' in out.stderr


def test_bench_dump_outputs(tmp_path, monkeypatch):
    """bench.py --dump-outputs: every array a step returns as <name>.npy in float64, integer values exact; an array beyond its
    share of the byte budget becomes the same seeded sample on every run, its positions stored beside it."""
    import bench
    monkeypatch.setattr(bench, 'DUMP_BYTES', 4096)
    rng = np.random.default_rng(5)
    out = dict(read_count=rng.integers(0, 2 ** 40, size=10), classes=rng.integers(0, 3, size=5000).astype(np.int8), n_rows=5000)
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), out)
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == sorted(os.listdir(tmp_path / 'b')) == ['classes.npy', 'classes_index.npy', 'n_rows.npy', 'read_count.npy']
    got = {n[:-4]: np.load(tmp_path / 'a' / n) for n in names}
    assert all(v.dtype == np.float64 for v in got.values())
    assert all(np.array_equal(v, np.load(tmp_path / 'b' / (k + '.npy'))) for k, v in got.items())
    assert sum(v.nbytes for v in got.values()) <= 4096
    assert np.array_equal(got['read_count'], out['read_count']) and got['n_rows'] == 5000
    pos = got['classes_index'].astype(np.int64)
    assert len(pos) == len(set(pos)) > 0 and np.array_equal(got['classes'], out['classes'][pos])


def test_bench_plain_run_skips_what_only_full_runs():
    """A plain bench.py run times its steps and nothing more; --full adds the resident-input steps, the single-worker pass, the
    output checks and the CPU baseline, each of which its own option still turns off."""
    import bench
    plain = bench.parse_args(['--steps', '3', '--resident-steps', '2', '--alone-reads', '512'])
    assert (plain.full, plain.resident_steps, plain.alone_reads, plain.no_correctness, plain.no_cpu_baseline) == (False, 0, -1, True, True)
    full = bench.parse_args(['--steps', '3', '--full'])
    assert (full.resident_steps, full.alone_reads, full.no_correctness, full.no_cpu_baseline) == (3, 0, False, False)
    full = bench.parse_args(['--steps', '3', '--full', '--resident-steps', '0', '--alone-reads', '-1', '--no-correctness', '--no-cpu-baseline'])
    assert (full.resident_steps, full.alone_reads, full.no_correctness, full.no_cpu_baseline) == (0, -1, True, True)


def test_classify_codes_equals_the_dataframe_classification():
    """filters.classify_codes (integer columns, bench.py --config c2) against filters.human_and_decoy_classify (the mirror of
    megapath_nano.py:1135-1200) on random tables."""
    import pandas as pd
    from megapath_nano_amd.filters import classify_codes, human_and_decoy_classify
    rng = np.random.default_rng(21)
    for trial in range(8):
        n_reads = int(rng.integers(5, 200))
        lens = rng.integers(300, 9000, size=n_reads)
        rows = []
        for r in range(n_reads):
            for _ in range(int(rng.integers(0, 4))):
                rows.append((r, int(rng.integers(0, 3)), int(rng.integers(100, 3000)), float(rng.random())))
        if not rows:
            continue
        ri, kind, sc, tb = (np.array(x) for x in zip(*rows))
        got = classify_codes(ri, kind, sc, tb, lens, n_reads)
        al = pd.DataFrame({'read_id': [f'r{r:04d}' for r in ri], 'read_length': lens[ri], 'assembly_id': [['H', 'D', 'M'][k] for k in kind],
                           'alignment_score': sc, 'alignment_score_tiebreaker': tb})
        out = human_and_decoy_classify(al, pd.DataFrame({'assembly_id': ['H']}), pd.DataFrame({'assembly_id': ['D']}),
                                       pd.DataFrame({'read_id': [f'r{r:04d}' for r in range(n_reads)], 'read_length': lens}))
        want = np.zeros(n_reads, dtype=np.int8)
        want[[int(x[1:]) for x in out['human_read_id_list']['read_id']]] = 1
        want[[int(x[1:]) for x in out['decoy_read_id_list']['read_id']]] = 2
        assert np.array_equal(got, want), trial
        assert len(out['microbe_read_id_list']) == int((want == 0).sum())
