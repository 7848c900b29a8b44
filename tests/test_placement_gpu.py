"""GPU tests (-m gpu) of the step between species placement and assembly selection: mapper.split_reads feeding the mapper with
device-resident group views, and placement.placement_to_assembly against the route the parent commit offers (fastx.nanosplit on
the host, one Align() per species file, pandas.concat) -- on a small strain-rich world made with synth.py: 3 species with a
species-ID assembly and two further candidates each, a species without candidates, and reads placed nowhere."""
import gzip
import os

import numpy as np
import pandas as pd
import pytest

import paf_check

pytestmark = pytest.mark.gpu

N_SPECIES = 3
OPTS = ['-N', '1000', '-p', '0', '-x', 'map-ont']


class Metadata:
    """assembly_metadata over an in-memory table: the joins Align() and placement_to_assembly use"""

    def __init__(self, table):
        self.t = table

    def _merge(self, assembly_list, cols, how):
        return assembly_list.merge(self.t[['assembly_id'] + cols].drop_duplicates(), on='assembly_id', how=how)

    def get_assembly_path(self, *, assembly_list, how='inner'):
        return self._merge(assembly_list[['assembly_id']], ['path'], how)

    def get_assembly_length(self, *, assembly_list, how='inner'):
        return self._merge(assembly_list[['assembly_id']], ['assembly_length'], how)

    def get_tax_id(self, *, assembly_list, how='inner'):
        return self._merge(assembly_list[['assembly_id']], ['tax_id', 'species_tax_id', 'genus_tax_id'], how)

    def get_sequence_tax_id(self, *, assembly_list, how='inner'):
        return self._merge(assembly_list[['assembly_id']], ['tax_id', 'species_tax_id', 'genus_tax_id', 'sequence_id'], how)


@pytest.fixture(scope='module')
def world(tmp_path_factory, libmpn, oracle_built):
    """Per species s: a root genome of 20-30 kb; the species-ID assembly (98 % of the root), candidate `true` (99.9 % of the root:
    the reads are drawn from it, so it is their 100 % assembly) and candidate `far` (97 % of the root).  Species 3 has a species-ID
    assembly only.  ~20 reads of 1-2 kb per species with candidates, 4 of species 3, 4 placed nowhere."""
    from megapath_nano_amd import synth
    d = tmp_path_factory.mktemp('placement')
    rng = np.random.default_rng(77)
    rows, genomes, reads, truth = [], {}, [], {}
    for s in range(N_SPECIES + 1):
        root = synth.random_genome(rng, int(rng.integers(20000, 30001)), gc=float(rng.uniform(0.4, 0.6)))
        kinds = [('id', 0.98)] + ([('true', 0.999), ('far', 0.97)] if s < N_SPECIES else [])
        for kind, ident in kinds:
            aid, sid = f'GCF_{s}{kind}.1', f'NZ_S{s}_{kind}.1'
            genomes[aid] = (sid, synth.mutate_strain(rng, root, ident))
            rows.append(dict(assembly_id=aid, path=f'{aid}.fna.gz', assembly_length=len(root), tax_id=1000 + 10 * s + len(rows) % 10,
                             species_tax_id=500 + s, genus_tax_id=50, sequence_id=sid, kind=kind))
            with gzip.open(d / f'{aid}.fna.gz', 'wb') as f:
                f.write(b'>' + sid.encode() + b' synthetic\n' + bytes(genomes[aid][1]) + b'\n')
        src = genomes[f'GCF_{s}true.1' if s < N_SPECIES else f'GCF_{s}id.1']
        for r in synth.make_reads(100 + s, [src], 20 if s < N_SPECIES else 4, mean_len=1500, min_len=1000, max_len=2000):
            name = f's{s}_{r["name"]}'
            reads.append((name, bytes(r['seq'])))
            truth[name] = 500 + s
    stray = [(f'stray{k}', bytes(synth.ALPHA[rng.integers(0, 4, size=1200)])) for k in range(4)]
    order = rng.permutation(len(reads) + len(stray))                   # the species are scattered over the batch
    reads = [(reads + stray)[i] for i in order]
    fq = d / 'run.fq'
    with open(fq, 'wb') as f:
        for k, (name, seq) in enumerate(reads):
            f.write(b'@' + name.encode() + (b' ch=%d' % k if k % 2 else b'') + b'\n' + seq + b'\n+\n' + bytes([33 + k % 40]) * len(seq) + b'\n')
    table = pd.DataFrame(rows)
    placed = pd.DataFrame({'read_id': [n for n, _ in reads if n in truth], 'species_tax_id': [truth[n] for n, _ in reads if n in truth]})
    # the species in an order of their own; 503 has no candidate assembly, 504 no assembly at all
    species_list = pd.DataFrame({'species_tax_id': [502, 500, 503, 501, 504], 'species_name': list('cadbe')})
    opts = dict(assembly_folder=str(d), min_alignment_score=0, debug=False, alignerThreadOption='-t 4', mapping_only=False)
    return dict(dir=d, table=table, meta=Metadata(table), genomes=genomes, reads=reads, fq=fq, placed=placed, species_list=species_list, opts=opts,
                species_id=table[table['kind'] == 'id'][['assembly_id']].reset_index(drop=True),
                # every assembly is a target; the species-ID ones were aligned against already and drop out (megapath_nano.py:1323-1330)
                targets=table[['assembly_id']].sample(frac=1, random_state=3).reset_index(drop=True))


@pytest.fixture(scope='module')
def resident(world):
    from megapath_nano_amd import mapper
    return mapper.PackedReads([n for n, _ in world['reads']], [s for _, s in world['reads']], device='cuda')


def _species_order(world):
    from megapath_nano_amd import placement
    by_species, species, placed = placement.candidate_tables(assembly_metadata=world['meta'], target_assembly_list=world['targets'],
                                                             species_id_assembly_id=world['species_id'], species_list=world['species_list'],
                                                             read_id_species_id=world['placed'])
    return by_species, species['species_tax_id'].tolist(), placed


def _genomes_of(world, by_species, species_tax_id):
    ids = by_species[by_species['species_tax_id'] == species_tax_id]['assembly_id']
    return [world['genomes'][a] for a in ids]


def test_candidate_tables(world):
    by_species, order, placed = _species_order(world)
    assert sorted(order) == [500, 501, 502] and by_species.shape[0] == 6                      # 503 has no candidate, 504 nothing
    assert set(by_species['assembly_id']) == {f'GCF_{s}{k}.1' for s in range(3) for k in ('true', 'far')}
    assert set(placed['species_tax_id']) == {500, 501, 502} and len(placed) == 60


def test_groups_of_a_resident_split_map_like_reads_packed_from_strings(world, resident):
    from megapath_nano_amd import mapper, placement
    by_species, order, placed = _species_order(world)
    split = placement.split_by_species([resident], placed, order)[0]
    seq_of = dict(world['reads'])
    opt = mapper.default_opt(best_n=1000, pri_ratio=0.0)
    for g, sp in enumerate(order):
        idx = mapper.Index(_genomes_of(world, by_species, sp))
        try:
            group = split.group(g)
            assert group.n == 20 and group.dev is not None and all(n.startswith(f's{sp - 500}_') for n in group.names)
            assert group.names == [n for n, _ in world['reads'] if n.startswith(f's{sp - 500}_')]            # input order
            plain = mapper.PackedReads(group.names, [seq_of[n] for n in group.names])
            got = mapper.map_batch_ex(idx, opt, group, want_paf=True, want_cols=True, use_device=True)
            want = mapper.map_batch_ex(idx, opt, plain, want_paf=True, want_cols=True, use_device=False)
            assert got[0] == want[0] and len(got[0]) > 0
            assert all(np.array_equal(got[1][c], want[1][c]) for c in mapper.COL_NAMES)
        finally:
            idx.close()


def _file_route(world, order, by_species):
    """what the parent commit offers: nanosplit on the host into one file per species, one Align() per file, concat in species order"""
    from megapath_nano_amd import fastx, placement
    from megapath_nano_amd.aligner import Align
    d = world['dir'] / 'split'
    d.mkdir(exist_ok=True)
    _, _, placed = _species_order(world)
    with open(d / 'read_query', 'w') as f:
        for read_id, sp in zip(placed['read_id'], placed['species_tax_id']):
            f.write(f'{read_id}\t{d / str(sp)}\n')
    fastx.nanosplit(str(d / 'read_query'), [str(world['fq'])], device=False)
    out = placement.empty_align_list()
    for sp in order:
        one = Align(assembly_metadata=world['meta'], global_options=world['opts'], temp_dir_name=str(d), log_file=None,
                    query_filename_list=pd.DataFrame([str(d / str(sp))], columns=['path']),
                    target_assembly_list=by_species[by_species['species_tax_id'] == sp], aligner_options=['-t', '4'] + OPTS,
                    mapping_only=world['opts']['mapping_only'])
        out = pd.concat([out, one], axis=0, sort=True)
    return out


@pytest.fixture(scope='module')
def tables(world, resident):
    from megapath_nano_amd import placement
    by_species, order, _ = _species_order(world)
    kw = dict(assembly_metadata=world['meta'], global_options=world['opts'], target_assembly_list=world['targets'],
              species_id_assembly_id=world['species_id'], species_list=world['species_list'], read_id_species_id=world['placed'])
    from_resident, n_candidates = placement.placement_to_assembly(reads=[resident], **kw)
    from_files, n2 = placement.placement_to_assembly(query_filename_list=pd.DataFrame({'path': [str(world['fq'])]}), **kw)
    return dict(resident=from_resident, files=from_files, route=_file_route(world, order, by_species), n=(n_candidates, n2))


def test_placement_to_assembly_equals_the_file_route(tables):
    assert tables['n'] == (6, 6)
    want = tables['route']
    assert len(want) > 60 and set(want['species_tax_id']) == {500, 501, 502}
    assert want['alignment_score_tiebreaker'].between(0, 1).all() and want['alignment_score_tiebreaker'].nunique() == len(want)
    for which in ('resident', 'files'):
        pd.testing.assert_frame_equal(tables[which], want, check_exact=True)       # rows, order, index, dtypes, tiebreakers


def test_a_species_paf_at_best_n_1000_equals_the_oracle(world, resident):
    from megapath_nano_amd import mapper, placement
    from oracle import mm2_bindings as mb
    by_species, order, placed = _species_order(world)
    group = placement.split_by_species([resident], placed, order)[0].group(0)
    gen = _genomes_of(world, by_species, order[0])
    idx, oidx = mapper.Index(gen), mb.Index(gen)
    try:
        paf, _ = mapper.map_batch_ex(idx, mapper.default_opt(best_n=1000, pri_ratio=0.0), group, want_paf=True, want_cols=False)
        oopt = mb.default_opt(best_n=1000, pri_ratio=0.0)
        want = ''.join(mb.map_read(oidx, oopt, n, group.seq(i).tobytes())[2] for i, n in enumerate(group.names))
    finally:
        idx.close()
        oidx.close()
    assert paf == want and paf.count('\n') >= 2 * group.n                # every read reaches both candidates
    paf_check.check_paf(paf, {n: group.seq(i).tobytes().decode() for i, n in enumerate(group.names)},
                        {name: bytes(seq).decode() for name, seq in gen}, best_n=1000)


def test_assembly_selection_picks_the_assembly_the_reads_came_from(world, tables):
    from megapath_nano_amd import abundance
    from megapath_nano_amd.aligner import Align
    species_align = Align(assembly_metadata=world['meta'], global_options=world['opts'], temp_dir_name=str(world['dir']), log_file=None,
                          query_filename_list=pd.DataFrame({'path': [str(world['fq'])]}), target_assembly_list=world['species_id'],
                          aligner_options=['-t', '4', '-N', '50', '-p', '1', '-x', 'map-ont'])
    t = world['table']
    sel = abundance.assembly_selection(species_align_list=species_align, assembly_align_list=tables['resident'], species_list=world['species_list'],
                                       read_id_species_id=world['placed'], assembly_ID_min_average_depth=0.1, good_align_threshold=100,
                                       assembly_length=t[['assembly_id', 'assembly_length']], assembly_tax=t[['assembly_id', 'tax_id', 'species_tax_id', 'genus_tax_id']])
    picked = dict(zip(sel.assembly_list['species_tax_id'], sel.assembly_list['assembly_id']))
    assert {s: picked[s] for s in (500, 501, 502)} == {500 + s: f'GCF_{s}true.1' for s in range(N_SPECIES)}
    assert picked.get(503) == 'GCF_3id.1'                               # no candidates: its species-ID assembly stays
