"""What the local realignment costs (megapath_nano_amd/local_realign.py), stage by stage, on the two shapes of
scripts/bench_create_tensor.py (its files; the positions are those our own candidate extraction finds, at most --max-sites of them,
evenly picked):

    genome     8 kb reads at 50x over 4 Mbp: shallow sites, many of them
    amplicon   50 000 reads of 1 kb on a 3 kb contig, 30 sites: every site meets samtools' -d 8000

    python scripts/bench_local_realign.py device [--scale S] [--max-sites N] [--chunks 4096,32768,...]     needs a GPU
    python scripts/bench_local_realign.py baseline <reference tree> --samtools PATH [--sites N]             CPU only
    python scripts/bench_local_realign.py readme                                                            writes the README

`device` times alt_info: the text resident (read, upload, inflate, flatten, walk), membership (host), columns and fragments, SSW, tally,
the host's text, and sweeps MPN_LR_SSW_CHUNK.  `baseline` runs the reference's own local_realignment.py, unmodified, once per position on
--sites evenly spaced positions of the same files (not the device run's sites) with a samtools built from the reference tree outside
this repository, on the CPU machine; `readme` extrapolates seconds a site to the device run's number of sites, which is rough with a
handful of positions: the code under test is never its own baseline.  The genome shape's sites are the candidate extraction's, a
superset of what the whole chain would call.  Both write a JSON file to profiles/r24_local_realign/;
`readme` writes profiles/r24_local_realign/README.md from them."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
OUT = os.path.join(ROOT, 'profiles', 'r24_local_realign')
STAGES = ('read', 'h2d', 'inflate', 'flatten', 'membership', 'columns_device_ms', 'fragments_device_ms', 'fragments', 'ssw_device_ms', 'tally_device_ms',
          'ssw_tally', 'host_text')


def pick_sites(positions, contig, max_sites, spaced):
    positions = np.asarray(positions, dtype=np.int64)
    positions = positions[(positions > 300) & (positions <= contig)]
    if len(positions) < spaced:
        return np.linspace(400, contig - 400, spaced).astype(np.int64), f'{spaced} evenly spaced (the extraction found {len(positions)})'
    if len(positions) > max_sites:
        return positions[np.linspace(0, len(positions) - 1, max_sites).astype(np.int64)], f'{max_sites} of the extraction\'s own {len(positions)}, evenly picked'
    return positions, 'the extraction\'s own'


def device(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_local_realign.py device needs a GPU')
    import bench_create_tensor as bct
    from megapath_nano_amd import local_realign
    res = {}
    for name in args.shapes.split(','):
        shape = bct.SHAPES[name]
        with tempfile.TemporaryDirectory() as d:
            bam_fn, ref_fn, _, genome, reads = bct.write_shape(d, name, shape, args.scale)
            sites, how = pick_sites(bct.own_candidates(name, bam_fn, ref_fn), shape['contig'], args.max_sites, 30)
            out = dict(reads=reads, contig=shape['contig'], sites=len(sites), positions=how, scale=args.scale)
            sweep, text = {}, None
            for chunk in [int(c) for c in args.chunks.split(',')]:
                os.environ['MPN_LR_SSW_CHUNK'] = str(chunk)
                runs = []
                for k in range(args.repeat + 1):
                    timings = {}
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    info = local_realign.alt_info(bam_fn, ref_fn, name, sites, timings=timings)
                    torch.cuda.synchronize()
                    timings['wall'] = time.perf_counter() - t0
                    lines = ''.join(local_realign.format_line(name, p, dp, m) for p, (dp, m) in info.items())
                    assert text in (None, lines)                       # the same bytes from run to run and from chunk to chunk
                    text = lines
                    if k:
                        runs.append(timings)
                sweep[str(chunk)] = {key: round(float(np.mean([r.get(key, 0) for r in runs])), 4) for key in STAGES + ('wall', 'pairs')}
                print(json.dumps({name: {chunk: sweep[str(chunk)]}}), file=sys.stderr, flush=True)
            out['sweep'] = sweep
            out['lines'] = text.count('\n')
            res[name] = out
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'device.json'), 'w') as f:
        json.dump(res, f)
    print(json.dumps(res))


def baseline(args):
    import bench_create_tensor as bct
    samtools = os.path.abspath(args.samtools)
    src = os.path.join(args.reference, 'bin', 'realignment')
    res = {}
    for name in args.shapes.split(','):
        shape = bct.SHAPES[name]
        with tempfile.TemporaryDirectory() as d:
            bam_fn, ref_fn, _, genome, reads = bct.write_shape(d, name, shape, args.scale)
            tool = os.path.join(d, 'realignment')
            os.makedirs(os.path.join(tool, 'realign'))
            for fn in ('local_realignment.py', 'fast_align_reads2ref.py', 'pyssw.py'):
                shutil.copy(os.path.join(src, fn), tool)
            subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-o', os.path.join(tool, 'realign', 'libssw.so'), os.path.join(src, 'realign', 'ssw.c'), '-lm'])
            subprocess.check_call([samtools, 'index', bam_fn])
            subprocess.check_call([samtools, 'faidx', ref_fn])
            sites = np.linspace(400, shape['contig'] - 400, args.sites).astype(np.int64)
            secs = []
            for pos in sites.tolist():
                t0 = time.perf_counter()
                subprocess.run([sys.executable, os.path.join(tool, 'local_realignment.py'), '--bam_fn', bam_fn, '--ref_fn', ref_fn, '--pos', str(pos), '--platform',
                                'ont', '--samtools', samtools, '--ctgName', name, '--output_fn', os.path.join(d, 'out')], check=True, capture_output=True)
                secs.append(time.perf_counter() - t0)
            res[name] = dict(reads=reads, scale=args.scale, sampled_sites=len(secs), seconds_per_site=round(float(np.mean(secs)), 3),
                             min=round(min(secs), 3), max=round(max(secs), 3), interpreter='CPython ' + sys.version.split()[0] + ' (the reference runs pypy3)')
            print(json.dumps({name: res[name]}), file=sys.stderr, flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'baseline.json'), 'w') as f:
        json.dump(res, f)
    print(json.dumps(res))


def readme(args):
    def load(fn):
        path = os.path.join(args.out, fn)
        return json.load(open(path)) if os.path.exists(path) else {}
    dev, base = load('device.json'), load('baseline.json')
    out = ['# Local realignment around called variants: what it costs', '',
           'Written by `scripts/bench_local_realign.py readme` from `device.json` (an MI355X) and `baseline.json` (the CPU machine). Numbers are',
           'recorded, not gated. Wall seconds unless a column says device ms (HIP events); means over the repeats after a warm-up run.', '']
    for name, d in dev.items():
        out += [f'## {name}: {d["reads"]} reads (scale {d["scale"]}), contig {d["contig"]}, {d["sites"]} sites ({d["positions"]}), {d["lines"]} lines', '',
                '| MPN_LR_SSW_CHUNK | pairs | wall s | text resident s | membership s | columns ms | fragments ms | SSW ms | tally ms | host text s |',
                '|---|---|---|---|---|---|---|---|---|---|']
        for chunk, t in d['sweep'].items():
            resident = t['read'] + t['h2d'] + t['inflate'] + t['flatten']
            out.append(f'| {chunk} | {int(t["pairs"])} | {t["wall"]:.3f} | {resident:.3f} | {t["membership"]:.3f} | {t["columns_device_ms"]:.1f} | '
                       f'{t["fragments_device_ms"]:.1f} | {t["ssw_device_ms"]:.1f} | {t["tally_device_ms"]:.1f} | {t["host_text"]:.3f} |')
        out.append('')
        if name in base:
            b = base[name]
            best = min(t['wall'] for t in d['sweep'].values())
            out += [f'The reference\'s own `local_realignment.py` (evenly spaced positions, not the sites above; unmodified, {b["interpreter"]}, samtools 1.13 built from the reference tree) on the CPU machine: '
                    f'{b["seconds_per_site"]} s a site on {b["sampled_sites"]} sampled sites ({b["min"]} .. {b["max"]}), one process at a time. Extrapolated to the '
                    f'{d["sites"]} sites above: {b["seconds_per_site"] * d["sites"]:.0f} s of one core, against {best:.2f} s here. The figure is an extrapolation from '
                    'the sample, and the reference spreads its processes over the cores it is given.', '']
    os.makedirs(args.out, exist_ok=True)
    path, notes = os.path.join(args.out, 'README.md'), ''
    if os.path.exists(path):                 # what was written by hand below the tables stays
        text = open(path).read()
        notes = text[text.index('\n## What the numbers say'):] if '\n## What the numbers say' in text else ''
    with open(path, 'w') as f:
        f.write('\n'.join(out) + notes)
    print('\n'.join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=('device', 'baseline', 'readme'))
    ap.add_argument('reference', nargs='?')
    ap.add_argument('--samtools')
    ap.add_argument('--shapes', default='amplicon,genome')
    ap.add_argument('--scale', type=float, default=1.0, help='fraction of the reads of each shape')
    ap.add_argument('--repeat', type=int, default=2)
    ap.add_argument('--max-sites', type=int, default=1 << 30)
    ap.add_argument('--sites', type=int, default=4, help='baseline: sites sampled per shape')
    ap.add_argument('--chunks', default='4096,32768,262144')
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    if args.what == 'baseline' and (not args.reference or not args.samtools):
        ap.error('baseline needs the reference tree and --samtools')
    dict(device=device, baseline=baseline, readme=readme)[args.what](args)


if __name__ == '__main__':
    main()
