"""Generates tests/golden/best_align_golden.json by IMPORTING the reference's /root/reference/bin/megapath_nano.py in this
container and running its align_list_to_best_align_list (:244-310), step_short_alignment_removal (:2293-2327) and
step_unique_alignment (:2553-2593) on the seeded tables of tests/best_cases.py, after random.seed(k).  Only seeds, digests of the
inputs and outputs are stored.

The module's imports that are not installed here (pybedtools, psutil, its own lib.*) are stubbed, and its
align_list_to_align_stat_by_assembly_id -- bedtools underneath -- is replaced by this package's host statement
align_stat_by_assembly_id(..., device=False): the abundance inside these goldens is OURS, everything around it is the reference's.

    python tests/golden/make_best_align_golden.py
"""
import importlib.util
import json
import os
import random
import sys
import types

import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from best_cases import LENGTHS, best_table, golden_cases, noise_bed_for, other_best_table, table_digest  # noqa: E402
from megapath_nano_amd.abundance import align_stat_by_assembly_id  # noqa: E402

REFERENCE = '/root/reference/bin/megapath_nano.py'


def load_reference():
    for name in ('pybedtools', 'pybedtools.bedtool', 'psutil', 'lib', 'lib.aligner', 'lib.reassignment', 'lib.assembly_metadata'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['pybedtools.bedtool'].BedTool = object
    sys.modules['lib.aligner'].Align = None
    sys.modules['lib.reassignment'].Reassign = None
    sys.modules['lib.assembly_metadata'].AssemblyMetadata = None
    spec = importlib.util.spec_from_file_location('reference_megapath_nano', REFERENCE)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    def stat(*, assembly_metadata, log, align_list, noise_bed=None):
        if align_list.shape[0] == 0:
            return pd.DataFrame({'assembly_id': [], 'adjusted_total_aligned_bp': []})
        return align_stat_by_assembly_id(align_list, assembly_metadata, None, noise_bed=noise_bed, device=False)
    ref.align_list_to_align_stat_by_assembly_id = stat
    return ref


class Log:
    def print(self, *a, **k):
        pass

    def print_time(self, *a, **k):
        pass


def main():
    ref = load_reference()
    mp = types.SimpleNamespace(log=Log(), output_folder='', output_prefix='', assembly_metadata=LENGTHS, global_options={'debug': False})
    out = []
    for k, case in enumerate(golden_cases()):
        table = best_table(**case['table'])
        noise = noise_bed_for(table, case['noise_seed']) if 'noise_seed' in case else None
        seed = 100 + k
        random.seed(seed)
        best = ref.align_list_to_best_align_list(assembly_metadata=LENGTHS, log=Log(), align_list=table, noise_bed=noise)
        next_random = random.random()                             # the stream position after the call
        rec = dict(name=case['name'], table=case['table'], noise_seed=case.get('noise_seed'), table_sha1=table_digest(table), seed=seed,
                   columns=list(best.columns), index=[int(i) for i in best.index],
                   tiebreaker=[float(x).hex() for x in best['alignment_score_tiebreaker']], next_random=next_random.hex())

        step = types.SimpleNamespace(I=types.SimpleNamespace(align_list=table, min_align_length=900), O=types.SimpleNamespace())
        random.seed(seed)
        ref.step_short_alignment_removal(mp, step)
        rec['short_alignment_removal'] = dict(min_align_length=900, index=[int(i) for i in step.O.align_list.index], columns=list(step.O.align_list.columns),
                                              num_read_before=int(step.O.num_read_before), num_read_after=int(step.O.num_read_after))

        human, decoy = other_best_table(table, 11 + k, 'human'), other_best_table(table, 31 + k, 'decoy')
        step = types.SimpleNamespace(I=types.SimpleNamespace(align_list=table, best_align_list=best, human_best_align_list=human, decoy_best_align_list=decoy,
                                                             unique_align_threshold=99.9), O=types.SimpleNamespace())
        ref.step_unique_alignment(mp, step)
        rec['unique_alignment'] = dict(human_seed=11 + k, decoy_seed=31 + k, unique_align_threshold=99.9, index=[int(i) for i in step.O.best_align_list.index],
                                       columns=list(step.O.best_align_list.columns),
                                       second_best=[int(x) for x in step.O.best_align_list['second_best_alignment_score']],
                                       num_read_before=int(step.O.num_read_before), num_read_after=int(step.O.num_read_after))
        out.append(rec)
        print(case['name'], 'rows', len(table), '->', len(best), 'reads;', 'short removal', rec['short_alignment_removal']['num_read_after'],
              'unique', rec['unique_alignment']['num_read_after'])
    with open(os.path.join(HERE, 'best_align_golden.json'), 'w') as f:
        json.dump(dict(source='reference bin/megapath_nano.py imported in the build container (pandas %s); the abundance statistic inside is this '
                              "package's align_stat_by_assembly_id(device=False)" % pd.__version__, cases=out), f, separators=(',', ':'))


if __name__ == '__main__':
    main()
