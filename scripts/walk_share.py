"""Queue time of the traceback and z-drop-test kernels in a rocprofv3 --kernel-trace run of bench.py, split by the kind of launch.
usage: python scripts/walk_share.py <kernel_trace.csv> <steps in the run> [out.txt]
Over the whole trace: per kernel (ext_bt_kernel, ext_ztest_kernel, ext_bt_wave_kernel, ext_ztest_wave_kernel) the launches and
their summed duration, the lane kernels split into small grids (at most 8 waves: the long lists of a group, and the second
pass) and large ones (the main lists); then the same per step, and as a share of the summed duration of all kernels (the busy
queue time: a queue runs one kernel at a time)."""
import collections
import csv
import sys

steps = float(sys.argv[2])
out = open(sys.argv[3], 'w') if len(sys.argv) > 3 else sys.stdout
tot, n, all_ns = collections.Counter(), collections.Counter(), 0
for r in csv.DictReader(open(sys.argv[1])):
    d = int(r['End_Timestamp']) - int(r['Start_Timestamp'])
    all_ns += d
    name = r['Kernel_Name'].split('(')[0].replace('void ', '').replace('mpn::', '')
    if not (name.startswith('ext_bt_') or name.startswith('ext_ztest_')):
        continue
    if 'wave' not in name:
        grid = int(r.get('Grid_Size_X') or r.get('Grid_Size') or 0)
        name += ' (small grid)' if grid <= 8 * 64 else ' (large grid)'
    tot[name] += d
    n[name] += 1
print(f'{steps:g} steps (warm-up included); all kernels {all_ns / 1e6:.1f} ms = {all_ns / 1e6 / steps:.1f} ms per step', file=out)
for k in sorted(tot):
    print(f'{k:36s} {n[k]:7d} launches {tot[k] / 1e6:9.1f} ms {tot[k] / 1e6 / steps:8.1f} ms/step {tot[k] / all_ns:.4f} of all kernel time '
          f'{tot[k] / n[k] / 1e3:8.1f} us/launch', file=out)
