"""What the averaging of Clair's lines per site and the overlap filter cost (megapath_nano_amd/clair_ensemble.py), stage by stage:
the host's grouping, resident probabilities to resident ensemble lines (wall, synchronised), the kernel's device time by HIP events
beside the bytes it must move, overlap_filter on formatted rows, and call_ensemble end to end beside the separate tools through text.

    genome K=1, K=4   96 470 one-line sites (the 4 Mbp / 50x shape of the earlier profiles), one model and four over one tensor block
    amplicon          30 sites of 88 lines (the 3 kb contig under 50 000 reads), one model
    mixed             100 000 one-line sites with one site of 400 lines among them: what a deep site costs a call of shallow ones

The blocks are drawn (seeded) on the device: the kernel's work does not depend on the values.  One JSON line.  The device part
cannot run without a GPU: there is no fallback.

    python scripts/bench_clair_ensemble.py [--e2e]
    python scripts/bench_clair_ensemble.py --reference-tree <reference tree> [--reference-lines N]     # CPU only: the reference's
                                           own ensemble.py under this Python on N drawn lines (one-line sites, and 88-line sites)
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
CELLS, PROBS = 1056, 90
HBM_ACHIEVABLE = 6.3e12       # bytes per second a streaming kernel reaches on an MI355X (8e12 is the specification)


def spread(values):
    return dict(mean=round(statistics.fmean(values), 5), min=round(min(values), 5), max=round(max(values), 5), n=len(values))


def kernel_case(name, centres, n_models, repeat):
    import torch
    from megapath_nano_amd import clair_ensemble
    centres = np.asarray(centres, dtype=np.int64)
    n = len(centres)
    g = torch.Generator(device='cuda').manual_seed(5)
    tensors = torch.randint(0, 60, (n, CELLS), dtype=torch.int32, device='cuda', generator=g)
    probs = [torch.rand((n, PROBS), dtype=torch.float32, device='cuda', generator=g) for _ in range(n_models)]
    runs, first = [], None
    for k in range(repeat + 1):
        t0 = time.perf_counter()
        lists = clair_ensemble.group(np.concatenate([centres] * n_models), (n_models + 2) // 2)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        sites, sums, means = clair_ensemble.ensemble(centres, tensors, probs, name, (n_models + 2) // 2)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        got = (sums.cpu().numpy().tobytes(), means.cpu().numpy().tobytes())
        assert first in (None, got)                    # bit-identical from run to run
        first = got
        if k:
            runs.append(dict(group_s=t1 - t0, ensemble_wall_s=t3 - t2, kernel_device_ms=clair_ensemble.last_device_ms()))
    lines, n_out = n * n_models, len(sites)
    requested = lines * (CELLS * 4 + PROBS * 4) + n_out * (CELLS * 4 + PROBS * 4) + lines * 8 + lists[0].nbytes + lists[2].nbytes
    compulsory = requested - (n_models - 1) * n * CELLS * 4          # a shared tensor row need come from HBM once
    out = dict(lines=lines, sites=n_out, models=n_models, bytes_requested=requested, bytes_compulsory=compulsory,
               bound_ms_at_6_3_TBps=round(compulsory / HBM_ACHIEVABLE * 1e3, 4), **{k: spread([r[k] for r in runs]) for k in runs[0]})
    out['kernel_GBps_of_requested'] = round(requested / (out['kernel_device_ms']['mean'] * 1e-3) / 1e9, 1)
    return out


def vcf_rows(n, seed=3):
    rng = random.Random(seed)
    rows, pos = [], 100
    for _ in range(n):
        pos += rng.randrange(1, 60)
        kind = rng.random()
        ref, alt = ('A', 'C') if kind < 0.7 else (('A' + 'C' * rng.randrange(1, 9), 'A') if kind < 0.85 else ('A', 'A' + 'T' * rng.randrange(1, 9)))
        q = rng.randrange(1, 900)
        rows.append('ctg\t%d\t.\t%s\t%s\t%d\tPASS\t.\tGT:GQ:DP:AF\t0/1:%d:%d:%.4f\n' % (pos, ref, alt, q, q, rng.randrange(4, 250), rng.random()))
    return rows


def overlap_case(n, repeat):
    from megapath_nano_amd import clair_ensemble
    rows = ['##fileformat=VCFv4.1\n', '#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n'] + vcf_rows(n)
    secs, kept = [], 0
    for _ in range(repeat):
        t0 = time.perf_counter()
        kept = len(clair_ensemble.overlap_filter(rows)) - 2
        secs.append(time.perf_counter() - t0)
    return dict(rows=n, kept=kept, overlap_filter_s=spread(secs))


def drawn_lines(keys, seed=9):
    rng = np.random.default_rng(seed)
    out = []
    for key in keys:
        cells = rng.integers(0, 60, CELLS)
        probs = rng.integers(0, 1000001, PROBS)
        out.append('\t'.join(['ctg', str(key), 'A' * 33] + [str(v) for v in cells.tolist()] + ['%d.%06d' % (v // 1000000, v % 1000000) for v in probs.tolist()]) + '\n')
    return ''.join(out)


def reference_runs(tree, n_lines):
    """the reference's own ensemble.py under this Python: seconds for n_lines one-line sites, and for n_lines lines of 88-line sites"""
    script = os.path.join(tree, 'bin', 'Clair-ensemble', 'Clair.beta.ensemble.cpu', 'clair', 'post_processing', 'ensemble.py')
    out = {}
    for name, keys in (('one_line_sites', list(range(n_lines))), ('sites_of_88_lines', [i // 88 for i in range(n_lines)])):
        text = drawn_lines(keys).encode()
        t0 = time.perf_counter()
        p = subprocess.run([sys.executable, script, '--minimum_count_to_output', '1'], input=text, capture_output=True, check=True)
        out[name] = dict(lines=n_lines, seconds=round(time.perf_counter() - t0, 3), lines_out=p.stdout.count(b'\n'), input_bytes=len(text))
    out['python'] = sys.version.split()[0]
    return out


def e2e(scale, n_models):
    """call_ensemble on the amplicon shape of scripts/bench_create_tensor.py beside the separate tools through text"""
    import bench_create_tensor as bct
    import clair_net_ref
    from test_clair_checkpoint import write_bundle
    from megapath_nano_amd import clair_ensemble
    with tempfile.TemporaryDirectory() as d:
        bam_fn, ref_fn, _, genome, reads = bct.write_shape(d, 'amplicon', bct.SHAPES['amplicon'], scale)
        prefixes = []
        for k in range(n_models):
            prefixes.append(os.path.join(d, 'model-%06d' % k))
            write_bundle(prefixes[-1], clair_net_ref.seeded_weights(30 + k))
        walls = []
        for k in range(2):                                   # the first run warms up
            timings = {}
            t0 = time.perf_counter()
            counts = clair_ensemble.call_ensemble(bam_fn, ref_fn, prefixes, 'amplicon', os.path.join(d, 'out%d' % k), rng=random.Random(1), timings=timings)
            walls.append(time.perf_counter() - t0)

        def tool(name, args, stdin):
            t0 = time.perf_counter()
            p = subprocess.run([sys.executable, os.path.join(ROOT, 'bin', name)] + args, input=stdin, capture_output=True, check=True)
            return p.stdout, time.perf_counter() - t0
        common = ['--bam_fn', bam_fn, '--ref_fn', ref_fn]
        steps = {}
        cand, steps['mpn-candidates'] = tool('mpn-candidates', common + ['--ctgName', 'amplicon'], b'')
        tens, steps['mpn-create-tensor'] = tool('mpn-create-tensor', common + ['--ctgName', 'amplicon'], cand)
        lines, steps['mpn-call-var'] = b'', 0.0
        for prefix in prefixes:
            part, s = tool('mpn-call-var', ['--chkpnt_fn', prefix, '--tensor_fn', 'PIPE', '--output_for_ensemble'], tens)
            lines, steps['mpn-call-var'] = lines + part, steps['mpn-call-var'] + s
        folded, steps['mpn-ensemble'] = tool('mpn-ensemble', ['--minimum_count_to_output', str((n_models + 2) // 2)], lines)
        vcf, steps['mpn-call-vcf'] = tool('mpn-call-vcf', common + ['--input_probabilities', '--pysam_for_all_indel_bases', '--sampleName', 'Amplicon'], folded)
        rows = vcf.decode().splitlines(keepends=True)
        body = sorted((r for r in rows if r[0] != '#'), key=lambda r: int(r.split('\t')[1]))
        _, steps['mpn-overlap-variant'] = tool('mpn-overlap-variant', [], ''.join([r for r in rows if r[0] == '#'] + body).encode())
        return dict(reads=reads, models=n_models, records=counts[0], after_filter=counts[1], call_ensemble_first_s=round(walls[0], 3),
                    call_ensemble_s=round(walls[1], 3), stages={k: round(v, 4) for k, v in timings.items() if isinstance(v, float)},
                    tools_through_text_s={k: round(v, 3) for k, v in steps.items()}, tools_sum_s=round(sum(steps.values()), 3),
                    text_bytes=dict(tensor_lines=len(tens), probability_lines=len(lines), ensemble_lines=len(folded)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--e2e', action='store_true', help='also call_ensemble beside the tools through text, on the amplicon shape')
    ap.add_argument('--e2e-scale', type=float, default=1.0)
    ap.add_argument('--e2e-models', type=int, default=2)
    ap.add_argument('--reference-tree', default=None, help='CPU only: time the reference\'s own ensemble.py of this tree and stop')
    ap.add_argument('--reference-lines', type=int, default=8800)
    args = ap.parse_args()
    if args.reference_tree:
        print(json.dumps(dict(reference_ensemble_py=reference_runs(args.reference_tree, args.reference_lines))))
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_clair_ensemble.py needs a GPU')
    res = {}
    res['genome_k1'] = kernel_case('genome', np.arange(96470) * 41 + 100, 1, args.repeat)
    res['genome_k4'] = kernel_case('genome', np.arange(96470) * 41 + 100, 4, args.repeat)
    res['amplicon'] = kernel_case('amplicon', np.repeat(np.arange(30) * 100 + 50, 88), 1, args.repeat)
    mixed = np.arange(100000) * 7 + 10
    res['mixed'] = kernel_case('mixed', np.concatenate([mixed[:50000], np.full(400, 5), mixed[50000:]]), 1, args.repeat)
    res['shallow_alone'] = kernel_case('mixed', mixed, 1, args.repeat)
    res['overlap_80000'] = overlap_case(80000, 3)
    res['overlap_5000'] = overlap_case(5000, 3)
    print(json.dumps(res), file=sys.stderr, flush=True)
    if args.e2e:
        res['e2e_amplicon'] = e2e(args.e2e_scale, args.e2e_models)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
