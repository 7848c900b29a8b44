"""What Clair's network costs from resident tensors to resident probabilities (megapath_nano_amd/clair_net.py), stage by stage: the
device time of the kernels by HIP events (the two input projections, the two recurrent passes, L3, L4, the small layers with the
softmaxes), the share of the 157.3 TFLOPS float32 matrix peak that the product-shaped stages reach, and the wall time of predict().

The tensors have the value distribution of the 4 Mbp case of scripts/bench_create_tensor.py: a stretch of that shape (8 kb reads at
50x, the ONT error mix) goes through the project's own candidate extraction and tensor creation, and the tensors it gives are
repeated up to --n (100 000; the 4 Mbp case has 96 470).  The wall time of those two stages on the stretch is reported beside the
network's on as many tensors, so that the share of the network in candidates -> tensors -> probabilities can be read off.  The
weights are seeded at the initialiser's scale (tests/clair_net_ref.py): the cost does not depend on them.

predict() runs --warmup times and then --repeat times; every figure comes with its spread.  Baseline: the float32 torch
restatement of the tests on the CPU (--threads, 16) on --cpu-sample tensors, scaled to --n.  One JSON line.  There is no fallback
without a GPU.

    python scripts/bench_clair_net.py
    python scripts/bench_clair_net.py --n 20000 --repeat 1 --no-cpu        # under a kernel trace, in a run of its own
"""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

PEAK_TFLOPS = 157.3
STRETCH = dict(contig=200_000, read_len=8_000, reads=1_250, sub_every=0)        # 50x, as the genome shape


def flops(n):
    """floating-point operations of the stages for n tensors (a multiply and an add each)"""
    return dict(project_ms=2.0 * 33 * n * (32 + 256) * 1024, recurrent_ms=2.0 * 2 * 33 * n * 128 * 1024, l3_ms=2.0 * n * 256 * 33 * 30,
                l4_ms=2.0 * n * 7680 * 192, heads_ms=2.0 * n * (192 * 384 + 96 * 90))


def spread(values):
    return dict(mean=round(statistics.fmean(values), 4), sd=round(statistics.pstdev(values), 4), min=round(min(values), 4), max=round(max(values), 4),
                n=len(values))


def stretch_tensors(timings):
    """the tensors of the stretch through candidates and clair_tensor -> an (m, 33, 8, 4) int32 tensor on the device"""
    import torch
    from bench_create_tensor import own_candidates, write_shape
    from megapath_nano_amd import clair_tensor
    with tempfile.TemporaryDirectory() as d:
        bam_fn, ref_fn, _, _, _ = write_shape(d, 'genome', STRETCH, 1.0)
        for k in range(2):                    # the first pass warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            positions = own_candidates('genome', bam_fn, ref_fn)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            _, block, _ = clair_tensor.tensors(bam_fn, ref_fn, positions, 'genome', rng=random.Random(1))
            torch.cuda.synchronize()
            t2 = time.perf_counter()
        timings.update(candidates_s=round(t1 - t0, 4), tensors_s=round(t2 - t1, 4), candidates=len(positions), tensors=block.shape[0])
    return block


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=100_000)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--cpu-sample', type=int, default=256)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--no-cpu', action='store_true', help='leave the CPU restatement out')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_clair_net.py needs a GPU')
    import clair_net_ref as ref
    from megapath_nano_amd import clair_net
    res = dict(n=args.n)
    stretch = {}
    sample = stretch_tensors(stretch)
    res['stretch'] = stretch
    m = sample.shape[0]
    x = sample.repeat((args.n + m - 1) // m, 1, 1, 1)[:args.n].contiguous()
    res['values'] = dict(max=int(sample.max()), mean=round(float(sample.float().mean()), 3), zero_share=round(float((sample == 0).float().mean()), 3))
    weights = ref.seeded_weights(7)
    net = clair_net.ClairNet(weights)
    res['chunk'], res['tile'] = net.chunk, clair_net.tile()
    out = torch.empty((args.n, 90), dtype=torch.float32, device='cuda')
    walls, stages, first = [], [], None
    for k in range(args.warmup + args.repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        probs = net.predict(x, out=out)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        if first is None:
            first = probs.clone()
        assert torch.equal(first, probs)              # the same bits from run to run
        if k >= args.warmup:
            walls.append(wall * 1e3)
            stages.append(clair_net.last_device_ms())
    res['wall_ms'] = spread(walls)
    res['device_ms'] = {k: spread([s[k] for s in stages]) for k in clair_net.STAGES}
    fl = flops(args.n)
    res['share_of_f32_matrix_peak'] = {k: round(fl[k] / (res['device_ms'][k]['mean'] * 1e-3) / (PEAK_TFLOPS * 1e12), 4) for k in ('project_ms', 'recurrent_ms', 'l4_ms')}
    res['tflops_overall'] = round(sum(fl.values()) / (res['device_ms']['total_ms']['mean'] * 1e-3) / 1e12, 2)
    # the stretch's own tensors, once: what the network adds to candidates -> tensors there
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    net.predict(sample)
    torch.cuda.synchronize()
    stretch['network_s'] = round(time.perf_counter() - t0, 4)
    stretch['network_share'] = round(stretch['network_s'] / (stretch['network_s'] + stretch['candidates_s'] + stretch['tensors_s']), 4)
    if not args.no_cpu:
        torch.set_num_threads(args.threads)
        sub = sample[:args.cpu_sample].cpu().numpy()
        ref.forward(weights, sub[:8], torch.float32)
        t0 = time.perf_counter()
        p32, _ = ref.forward(weights, sub, torch.float32)
        cpu = time.perf_counter() - t0
        res['cpu_float32'] = dict(threads=args.threads, tensors=len(sub), seconds=round(cpu, 3), scaled_to_n_s=round(cpu * args.n / len(sub), 1),
                                  max_abs_difference=float(np.abs(p32 - first[:len(sub)].cpu().numpy()).max()))
    net.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
