"""Times ext_dp_batch on seeded sets of long extension windows, kernel by kernel (force_kernel 5 = band kernel, 6 = tiled where
eligible).  Run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python3 scripts/tile_bench.py ...` for per-kernel times; it
prints the wall time per call itself.  MPN_TILE_CLASS picks the tiled class (plan_kernels.h tile_class_*).

  sets: ext5k   10 x ~5000 x 5000, w = 751, EXTZ (one band<8,2> launch's worth)
        fill1k6 64 x 1600 x 1600, w = 750, approximate maximum (gap fills)
        mix     both in one call"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
APPROX, EXTZ = 0x02, 0x40


def make_set(name, seed=7):
    from test_ext_dp_gpu import mutate
    rng = np.random.default_rng(seed)

    def pairs(n, L, rate, tail):
        qs, ts = [], []
        for _ in range(n):
            t = rng.integers(0, 4, size=L).astype(np.uint8)
            q = mutate(rng, t, rate)[:L]
            if tail:   # unrelated ends: the extension z-drops somewhere past the homologous part
                q = np.concatenate([q, rng.integers(0, 4, size=200).astype(np.uint8)])
                t = np.concatenate([t, rng.integers(0, 4, size=200).astype(np.uint8)])
            qs.append(q)
            ts.append(t)
        return qs, ts
    if name == 'ext5k':
        qs, ts = pairs(10, 4800, 0.1, True)
        return qs, ts, [751] * 10, [EXTZ] * 10
    if name == 'fill1k6':
        qs, ts = pairs(64, 1600, 0.1, False)
        return qs, ts, [750] * 64, [APPROX] * 64
    a, b = make_set('ext5k', seed), make_set('fill1k6', seed + 1)
    return a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + b[3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sets', default='ext5k,fill1k6,mix')
    ap.add_argument('--kernels', default='5,6')
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    from megapath_nano_amd import mapper
    opt = mapper.default_opt()
    out = {'tile_class': os.environ.get('MPN_TILE_CLASS', 'auto')}
    for name in args.sets.split(','):
        qs, ts, w, fl = make_set(name)
        ref = None
        for k in [int(x) for x in args.kernels.split(',')]:
            # (one flag per call: the sets with two flags go in two calls back to back, like the two launches they stand for)
            groups = sorted(set(fl))
            def run():
                res = []
                for f in groups:
                    ix = [i for i in range(len(qs)) if fl[i] == f]
                    res += mapper.ext_dp_batch(opt, [qs[i] for i in ix], [ts[i] for i in ix], [w[i] for i in ix], 400, -1, f, force_kernel=k)
                return res
            got = run()   # warm-up (code objects, pools)
            t0 = time.perf_counter()
            for _ in range(args.reps):
                run()
            dt = (time.perf_counter() - t0) / args.reps
            same = ref is None or got == ref
            ref = ref or got
            out[f'{name}/k{k}'] = {'ms_per_call': round(dt * 1e3, 2), 'same_as_first_kernel': same}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
