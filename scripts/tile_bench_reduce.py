"""Per-set DP kernel time of a `rocprofv3 --kernel-trace` run of scripts/tile_bench.py with its default arguments (first call of each
set and kernel is the warm-up)."""
import csv, sys
rows=sorted(csv.DictReader(open(sys.argv[1])), key=lambda r:int(r['Start_Timestamp']))
dp=[(r['Kernel_Name'].split('(')[0].replace('void mpn::','').replace('mpn::',''), (int(r['End_Timestamp'])-int(r['Start_Timestamp']))/1e6, r['VGPR_Count'], r['LDS_Block_Size'], r['Workgroup_Size_X'], r['Grid_Size_X']) for r in rows if 'ext_dp_' in r['Kernel_Name']]
# order: ext5k band x4, tile x4; fill band x4, tile x4; mix (band,band) x4, (tile,tile) x4 ; first of each 4 is warm-up
seq=[('ext5k',1),('ext5k',1),('fill1k6',1),('fill1k6',1),('mix',2),('mix',2)]
i=0
for name,per in seq:
    calls=[dp[i+k*per:i+(k+1)*per] for k in range(4)]; i+=4*per
    kern=calls[0][0][0] if per==1 else '+'.join(c[0] for c in calls[0])
    ms=[sum(c[1] for c in call) for call in calls[1:]]
    print(f'{name:8s} {kern:40s} ms/call (timed reps) {" ".join(f"{m:6.2f}" for m in ms)}  vgpr {calls[0][0][2]} lds {calls[0][0][3]} wg {calls[0][0][4]} grid {calls[0][0][5]}')
