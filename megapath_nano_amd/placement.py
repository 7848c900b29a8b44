"""Host-side mirror of the reference's step_placement_to_assembly (/root/reference/bin/megapath_nano.py:1313-1397): the reads
species placement put into a species are mapped against that species' further candidate assemblies, one mapping call per species
at `-N 1000 -p 0 -x map-ont`.  The table it returns is the `assembly_align_list` of abundance.assembly_selection.

What differs from the reference: no files and no child processes in between.  The reference writes a `read_id <TAB> file` list,
has bin/tools/nanosplit cut the run's FASTQ into one file per species and starts one Align() per file; here the run's reads are
(or become) resident in HBM, mapper.split_reads regroups them by species on the device, and every species' group -- a view of the
one regrouped buffer -- is mapped where it lies.  The rows go through the same code as Align()'s (aligner.align_table), with
`random` seeded as Align() would seed it for a query file named after the species.
"""
import hashlib
import random
import shlex

import numpy as np
import pandas

from . import aligner, mapper

# the columns and types of the table the reference starts its concatenation from (megapath_nano.py:110-115,:1366-1368)
ALIGN_LIST_TYPES = {'read_id': str, 'read_length': int, 'read_from': int, 'read_to': int, 'strand': str, 'sequence_id': str, 'sequence_length': int,
                    'sequence_from': int, 'sequence_to': int, 'match': int, 'mapq': int, 'edit_dist': int, 'alignment_score': int, 'assembly_id': str,
                    'tax_id': int, 'species_tax_id': int, 'genus_tax_id': int, 'alignment_score_tiebreaker': float}
ALIGNER_OPTIONS = ' -N 1000 -p 0 -x map-ont'


def empty_align_list():
    table = pandas.DataFrame(columns=list(ALIGN_LIST_TYPES))
    for col, kind in ALIGN_LIST_TYPES.items():
        table[col] = table[col].astype(kind)
    return table


def candidate_tables(*, assembly_metadata, target_assembly_list, species_id_assembly_id, species_list, read_id_species_id):
    """The three merges of megapath_nano.py:1323-1350, one row per assembly or read: the target assemblies that were not aligned
    against already (the species-ID set), with their taxonomy, of the species that were selected; those species in the order of
    their first candidate; and the reads placed in one of them.  -> (species_target_assembly_list, species, read_id_species_id)"""
    aligned = species_id_assembly_id.assign(aligned=lambda x: 1).set_index('assembly_id')
    candidates = target_assembly_list.merge(right=aligned, how='left', left_on='assembly_id', right_index=True, suffixes=['', '_y'], validate='1:1')
    candidates = candidates.fillna(0).query('aligned == 0').drop(['aligned'], axis=1)
    by_species = assembly_metadata.get_tax_id(assembly_list=candidates).merge(right=species_list[['species_tax_id']].set_index('species_tax_id'), how='inner',
                                                                                left_on='species_tax_id', right_index=True, suffixes=['', '_y'], validate='m:1')
    species = by_species[['species_tax_id']].drop_duplicates()
    placed = read_id_species_id.merge(right=species.set_index('species_tax_id'), how='inner', left_on='species_tax_id', right_index=True,
                                      suffixes=['', '_y'], validate='m:1')
    return by_species, species, placed


def split_by_species(batches, placed, species_ids):
    """Every batch regrouped by species (group g = species_ids[g]): the reads are matched by name like nanosplit matches them, a
    name that occurs twice is taken twice.  -> list of mapper.ReadSplit, one per batch"""
    group_of = pandas.DataFrame({'species_tax_id': list(species_ids), 'group': np.arange(len(species_ids), dtype=np.int32)})
    pairs = placed[['read_id', 'species_tax_id']].merge(group_of, on='species_tax_id', how='inner')[['read_id', 'group']]
    splits = []
    for b in batches:
        mine = pandas.DataFrame({'read_id': b.names, 'read_idx': np.arange(b.n, dtype=np.int32)}).merge(pairs, on='read_id', how='inner')
        splits.append(mapper.split_reads(b, mine['read_idx'].to_numpy(dtype=np.int32), mine['group'].to_numpy(dtype=np.int32), len(species_ids)))
    return splits


def placement_to_assembly(*, assembly_metadata, global_options, target_assembly_list, species_id_assembly_id, species_list, read_id_species_id,
                          query_filename_list=None, reads=None, batch_bases=200_000_000, device='cuda'):
    """step_placement_to_assembly.  target_assembly_list: DataFrame(assembly_id), the candidate assemblies; species_id_assembly_id:
    DataFrame(assembly_id, ...) the assemblies species placement aligned against already; species_list: DataFrame(species_tax_id),
    the selected species; read_id_species_id: DataFrame(read_id, species_tax_id); assembly_metadata: get_tax_id, get_assembly_path,
    get_assembly_length, get_sequence_tax_id; global_options: alignerThreadOption, mapping_only, assembly_folder, min_alignment_score.
    The reads: query_filename_list (DataFrame(path), read into HBM here) or `reads`, a list of mapper.PackedReads that are resident.
    -> (align_list, num_assembly_candidate)

    A species that has candidate assemblies but no placed read is skipped; the reference stops there in Align() ("Query file ...
    not exists"), because nanosplit never created that species' file."""
    if (query_filename_list is None) == (reads is None):
        raise ValueError('placement_to_assembly: exactly one of query_filename_list and reads')
    by_species, species, placed = candidate_tables(assembly_metadata=assembly_metadata, target_assembly_list=target_assembly_list,
                                                    species_id_assembly_id=species_id_assembly_id, species_list=species_list,
                                                    read_id_species_id=read_id_species_id)
    species_ids = species['species_tax_id'].tolist()
    if reads is None:
        reads = list(aligner.iter_read_batches([str(p) for p in query_filename_list['path']], batch_bases, device=device))
    splits = split_by_species(reads, placed, species_ids)
    options = aligner.AlignerOptions(shlex.split(global_options['alignerThreadOption'] + ALIGNER_OPTIONS), global_options['mapping_only'])
    align_list = empty_align_list()
    for g, species_tax_id in enumerate(species_ids):
        groups = [s.group(g) for s in splits if s.n_reads(g)]
        if not groups:
            continue
        targets = by_species[(by_species['species_tax_id'] == species_tax_id).to_numpy()]
        # the tiebreaker stream of an Align() whose one query file is named after the species (aligner.py:160-168)
        random.seed(hashlib.md5(str(species_tax_id).encode()).hexdigest())
        paths = aligner._resolve_targets(assembly_metadata, global_options, None, targets, False, '')
        batches = []
        if aligner.target_ingest_on_device(paths):   # MPN_TARGET_INGEST=device: the parts arrive built (ingest.py)
            from . import ingest
            parts = ingest.iter_target_parts_device(paths, options.batch_bases, k=options.k, w=options.w)
        else:
            parts = aligner.iter_target_parts(aligner.iter_target_records(paths), options.batch_bases)
        for part in parts:
            idx = part if isinstance(part, mapper.Index) else mapper.Index(part, k=options.k, w=options.w)
            try:   # an exception must not leave the species' index in HBM
                names, lens = np.array(idx.names, dtype=object), idx.lens
                for p in groups:
                    _, _, cols = mapper.map_batch_full(idx, options.opt, p, want_paf=False, want_cols=True)
                    batches.append(aligner.MappedBatch(p, None, None, cols, names, lens))
            finally:
                idx.close()
        table = aligner.align_table(batches, assembly_metadata=assembly_metadata, global_options=global_options, target_assembly_list=targets)
        align_list = pandas.concat([align_list, table], axis=0, sort=True)
    return align_list, int(by_species.shape[0])
