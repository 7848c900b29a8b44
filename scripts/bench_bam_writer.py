"""The three BAM writers on the SAM of a 100 000-read Align() (bench_align.py's input and options), and Align() with files under each:

  host      bam.sam_to_sorted_bam with the device sort and zlib (Align()'s default)
  bgzf      the same with compress_blocks=bam.device_bgzf_blocks (MPN_BGZF=device)
  device    bam.sam_to_sorted_bam_device (MPN_BAM_WRITER=device): records resident from the SAM text to the deflated blocks

One Align() with files makes the .sam (and warms the library up); the writers then run on it --rounds times, alternated, in this
process.  The device writer's stages are reported from its own clocks (HIP events for scan, encode, gather, deflate; host clocks
around returned calls for the rest).  Then Align() with files is timed --rounds times under each setting, alternated.  One JSON line.

  python scripts/bench_bam_writer.py [--reads 100000] [--rounds 3] [--out profiles/r27_bam_writer/bench_bam_writer_100k.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))


def spread(v):
    return {'median': round(sorted(v)[len(v) // 2], 3), 'min': round(min(v), 3), 'max': round(max(v), 3), 'all': [round(x, 3) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=100000)
    ap.add_argument('--genomes', type=int, default=5)
    ap.add_argument('--genome-len', type=int, default=5000000)
    ap.add_argument('--mean-len', type=int, default=8000)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--extra', default='')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import pandas as pd
    from bench_align import write_inputs
    from megapath_nano_amd import abundance, aligner, bam, build
    build.build()
    opts = ['-t', '16', '-I', '8G', '-N', '50', '-p', '1', '-x', 'map-ont', '--split-prefix', 'tmp'] + args.extra.split()
    for k in ('MPN_BGZF', 'MPN_BAM_WRITER'):
        os.environ.pop(k, None)
    with tempfile.TemporaryDirectory(dir=os.environ.get('TMPDIR', '/tmp')) as d:
        paths, fq, bases = write_inputs(d, args.genomes, args.genome_len, args.reads, args.mean_len, 77)
        tf, qf = pd.DataFrame({'path': paths}), pd.DataFrame({'path': [fq]})

        def align(prefix):
            t0 = time.perf_counter()
            aligner.Align(assembly_metadata=None, global_options={'min_alignment_score': 0}, temp_dir_name=d, log_file=sys.stderr, query_filename_list=qf,
                          target_filename_list=tf, aligner_options=opts, paf_path_and_prefix=prefix)
            return time.perf_counter() - t0
        align(os.path.join(d, 'warm'))
        sam = os.path.join(d, 'warm.sam')
        out = {'reads': args.reads, 'read_bases': bases, 'sam_bytes': os.path.getsize(sam), 'rounds': args.rounds, 'extra': args.extra}

        def writer(kind, path):
            t0 = time.perf_counter()
            if kind == 'device':
                n = bam.sam_to_sorted_bam_device(sam, path, exclude_flags=1796)
            else:
                n = bam.sam_to_sorted_bam(sam, path, exclude_flags=1796, sort_keys=abundance.device_sort_order,
                                          compress_blocks=bam.device_bgzf_blocks if kind == 'bgzf' else None)
            return time.perf_counter() - t0, n

        # the device writer once more through the builder, for its stage clocks
        def staged(path):
            header = []
            with open(sam, 'rb') as f:
                for raw in f:
                    if raw[:1] != b'@':
                        break
                    header.append(raw.decode())
                names, lens = bam.parse_header(header)
                b = bam.DeviceBamBuilder(names, lens, bam.sorted_header_text(header), 1796)
                f.seek(0)
                t0 = time.perf_counter()
                read_s = 0.0
                while True:
                    t1 = time.perf_counter()
                    data = f.read(1 << 28)
                    read_s += time.perf_counter() - t1
                    if not data:
                        break
                    b.add_text(data)
                b.finish(path)
                total = time.perf_counter() - t0
            ms = b.stage_ms()
            b.close()
            return {'total_s': round(total, 3), 'file_read_s': round(read_s, 3), **{k + '_s': round(v / 1e3, 3) for k, v in ms.items()}}

        writer('device', os.path.join(d, 'w0.bam'))           # warm-up of the new path
        times = {'host': [], 'bgzf': [], 'device': []}
        for r in range(args.rounds):
            for kind in times:
                t, n = writer(kind, os.path.join(d, f'w_{kind}.bam'))
                times[kind].append(t)
                out['records'] = int(n)
        out['writer_s'] = {k: spread(v) for k, v in times.items()}
        out['bam_bytes'] = {k: os.path.getsize(os.path.join(d, f'w_{k}.bam')) for k in times}
        out['identical_bgzf_device'] = all(open(os.path.join(d, f'w_bgzf.bam{e}'), 'rb').read() == open(os.path.join(d, f'w_device.bam{e}'), 'rb').read()
                                           for e in ('', '.bai'))
        out['device_stages'] = [staged(os.path.join(d, 'w_staged.bam')) for _ in range(args.rounds)]
        calls = {'host': [], 'bgzf': [], 'device': []}
        for r in range(args.rounds):
            for kind in calls:
                for k in ('MPN_BGZF', 'MPN_BAM_WRITER'):
                    os.environ.pop(k, None)
                if kind == 'bgzf':
                    os.environ['MPN_BGZF'] = 'device'
                if kind == 'device':
                    os.environ['MPN_BAM_WRITER'] = 'device'
                calls[kind].append(align(os.path.join(d, f'a_{kind}')))
        out['align_with_files_s'] = {k: spread(v) for k, v in calls.items()}
        out['align_identical_bgzf_device'] = all(open(os.path.join(d, f'a_bgzf.bam{e}'), 'rb').read() == open(os.path.join(d, f'a_device.bam{e}'), 'rb').read()
                                                 for e in ('', '.bai'))
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
