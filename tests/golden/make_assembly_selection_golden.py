"""Generates tests/golden/assembly_selection_golden.json by IMPORTING the reference's /root/reference/bin/megapath_nano.py in this
container and running its good_align_list (:642-663), align_list_to_align_stat_by_sequence_id (:585-639) and
step_assembly_selection (:1400-1476, with align_list_to_align_stat_by_assembly_id, summary_stat_1 and summary_stat_2 as the
reference wrote them) on the seeded tables of tests/select_cases.py.

Stubbed is only what needs bedtools or the metadata database: align_list_to_bed hands the alignments on, and the two
bed_to_covered_bp_* functions return this package's host covered bp (covered_bp_by_assembly / host_cover_by_group) or, for a noise
BED, the plain sum of its intervals; a small assembly_metadata object does the left merges for the lengths and the tax ids.  The
grouped sums and every derived column in these goldens are the reference's own pandas.

    python tests/golden/make_assembly_selection_golden.py
"""
import json
import os
import sys
import types

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_best_align_golden import REFERENCE, Log, load_reference as load_with_stubs  # noqa: E402
from select_cases import frame_record, inputs_digest, selection_cases, selection_inputs  # noqa: E402
from megapath_nano_amd import abundance  # noqa: E402


class Bed:
    """what stands for a BedTool: the alignments behind a covered BED (and the noise subtracted from it), or a noise BED's frame"""
    def __init__(self, rows=None, noise=None, frame=None):
        self.rows, self.noise, self.frame = rows, noise, frame

    def subtract(self, other):
        return Bed(rows=self.rows, noise=other.frame)


def covered_by_assembly(*, bed):
    if bed.frame is not None:
        f = bed.frame
        return f.assign(covered_bp=f['end'] - f['start'])[['assembly_id', 'covered_bp']].groupby(['assembly_id'], as_index=False).sum()
    cov = abundance.covered_bp_by_assembly(bed.rows, noise_bed=bed.noise, device=False)
    return pd.DataFrame({'assembly_id': list(cov), 'covered_bp': np.array(list(cov.values()), dtype=np.int64)})


def covered_by_sequence(*, bed):
    if bed.frame is not None:
        f = bed.frame
        return f.assign(covered_bp=f['end'] - f['start'])[['sequence_id', 'covered_bp']].groupby(['sequence_id'], as_index=False).sum()
    seqs, sc = abundance._codes(bed.rows['sequence_id'])
    sc = sc.astype(np.int32)
    start, end = bed.rows['sequence_from'].to_numpy(dtype=np.int64), bed.rows['sequence_to'].to_numpy(dtype=np.int64)
    cov = abundance.host_cover_by_group(sc, sc, start, end, len(seqs))
    if bed.noise is not None:                                    # |A \ N| = |A u N| - |N| on the sequences that carry alignments
        where = pd.Index(seqs).get_indexer(bed.noise['sequence_id'])
        hit = where >= 0
        nk, ns, ne = where[hit].astype(np.int32), bed.noise['start'].to_numpy(dtype=np.int64)[hit], bed.noise['end'].to_numpy(dtype=np.int64)[hit]
        both = np.concatenate([sc, nk])
        cov = (abundance.host_cover_by_group(both, both, np.concatenate([start, ns]), np.concatenate([end, ne]), len(seqs)) -
               abundance.host_cover_by_group(nk, nk, ns, ne, len(seqs)))
    return pd.DataFrame({'sequence_id': seqs, 'covered_bp': cov})


class Metadata:
    def __init__(self, inp):
        self.length = inp['assembly_length'].set_index('assembly_id')
        self.tax = inp['assembly_tax'].set_index('assembly_id')
        self.sequence = inp['sequence_length'].set_index('sequence_id')

    def _merge(self, left, right, on, how):
        return left.merge(right=right, how=how, left_on=on, right_index=True, suffixes=['', '_y'], validate='m:1')

    def get_assembly_length(self, *, assembly_list, how='inner'):
        return self._merge(assembly_list, self.length, 'assembly_id', how)

    def get_tax_id(self, *, assembly_list, how='inner'):
        return self._merge(assembly_list, self.tax, 'assembly_id', how)

    def get_sequence_length(self, *, sequence_list, how='inner'):
        return self._merge(sequence_list, self.sequence, 'sequence_id', how)


def load_reference():
    import importlib.util
    load_with_stubs()                                            # leaves the stubs of pybedtools, psutil and lib.* in sys.modules
    spec = importlib.util.spec_from_file_location('reference_megapath_nano_selection', REFERENCE)
    ref = importlib.util.module_from_spec(spec)                  # a copy of its own: the by-assembly statistic stays the reference's
    spec.loader.exec_module(ref)
    ref.align_list_to_bed = lambda *, align_list: Bed(rows=align_list)
    ref.bed_to_covered_bp_by_assembly_id = covered_by_assembly
    ref.bed_to_covered_bp_by_sequence_id = covered_by_sequence
    return ref


def main():
    ref = load_reference()
    out = []
    for case in selection_cases():
        inp = selection_inputs(case)
        meta = Metadata(inp)
        mp = types.SimpleNamespace(log=Log(), output_folder='', output_prefix='', assembly_metadata=meta, global_options={'debug': False})
        species = inp['species_align_list']
        rec = dict(case=case, tables_sha1=inputs_digest(inp))
        rec['good_align_list'] = frame_record(ref.good_align_list(align_list=species, good_align_threshold=case['threshold']), values=False)
        noise = Bed(frame=inp['noise_bed']) if inp['noise_bed'] is not None else None
        rec['align_stat_by_sequence_id'] = frame_record(ref.align_list_to_align_stat_by_sequence_id(assembly_metadata=meta, log=Log(), align_list=species,
                                                                                                     noise_bed=noise))
        step = types.SimpleNamespace(I=types.SimpleNamespace(species_align_list=species, assembly_align_list=inp['assembly_align_list'],
                                                             species_list=inp['species_list'], read_id_species_id=inp['read_id_species_id'],
                                                             assembly_ID_min_average_depth=case['min_depth'], good_align_threshold=case['threshold']),
                                     O=types.SimpleNamespace())
        ref.step_assembly_selection(mp, step)
        for name in ('align_list', 'best_align_list', 'good_align_list'):
            rec['selection_' + name] = frame_record(getattr(step.O, name), values=False)
        rec['selection_align_stat'] = frame_record(step.O.align_stat)
        rec['selection_assembly_list'] = frame_record(step.O.assembly_list)
        out.append(rec)
        print(case['name'], 'rows', len(species), '+', len(inp['assembly_align_list']), '->', len(step.O.align_list), 'selected,', len(step.O.good_align_list), 'good,',
              len(step.O.assembly_list), 'assemblies;', dict(zip(step.O.align_stat['assembly_id'], step.O.align_stat['adjusted_average_depth'].round(3))))
    with open(os.path.join(HERE, 'assembly_selection_golden.json'), 'w') as f:
        json.dump(dict(source='reference bin/megapath_nano.py imported in the build container (pandas %s); covered bp from this package\'s host '
                              'statements, everything else the reference\'s own functions' % pd.__version__, cases=out), f, separators=(',', ':'))


if __name__ == '__main__':
    main()
