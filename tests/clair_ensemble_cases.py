"""Inputs of the ensemble tests (test infrastructure): the goldens of the reference's own scripts, the case file of the host build
(scripts/clair_ensemble_host_check.cpp) and its result, the same for tests/test_clair_ensemble_host.py and the GPU tests."""
import functools
import gzip
import json
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'clair_ensemble', 'clair_ensemble_golden.json.gz')
CELLS, PROBS = 1056, 90
ENSEMBLE_NAMES = ['one_line_per_key', 'counts', 'interleaved_min0', 'interleaved_min1', 'interleaved_min2', 'interleaved_min3', 'interleaved_min4',
                  'odd_sums', 'ties', 'thirds_and_sevenths', 'wide_values']
OVERLAP_NAMES = ['deletion_over_snp', 'chains', 'two_alts', 'insertions_and_edges', 'chromosomes_and_quals', 'header_only', 'no_header']


@functools.lru_cache(maxsize=None)
def golden():
    with gzip.open(GOLDEN, 'rb') as f:
        return json.load(f)


def ensemble_case(name):
    return next(c for c in golden()['ensemble'] if c['name'] == name)


def overlap_case(name):
    return next(c for c in golden()['overlap'] if c['name'] == name)


def build_host_check(out_dir):
    """g++ under AddressSanitizer and UBSan, contraction off (csrc/clair_ensemble_core.h says why) -> the program"""
    out = os.path.join(str(out_dir), 'clair_ensemble_host_check')
    subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    '-o', out, os.path.join(ROOT, 'scripts', 'clair_ensemble_host_check.cpp')], check=True)
    return out


def grouping(keys, minimum_count):
    """the sites of a list of keys in order of first appearance -> (site_off, site_lines, out_slot, n_out, the first line of every site)"""
    lines = {}
    for i, k in enumerate(keys):
        lines.setdefault(k, []).append(i)
    site_off, site_lines, out_slot, n_out = [0], [], [], 0
    for k, ls in lines.items():
        site_lines += ls
        site_off.append(len(site_lines))
        out_slot.append(n_out if len(ls) >= minimum_count else -1)
        n_out += len(ls) >= minimum_count
    return site_off, site_lines, out_slot, n_out, [ls[0] for ls in lines.values()]


def case_bytes(tensor_row, prob_row, tensors, probs, site_off, site_lines, out_slot, n_out, n_entries=None):
    tensors = np.ascontiguousarray(tensors, dtype=np.int32).reshape(-1, CELLS)
    probs = np.ascontiguousarray(probs).reshape(-1, PROBS)
    assert probs.dtype in (np.float32, np.float64)
    head = struct.pack('<7q', len(tensor_row), len(tensors), len(probs), int(probs.dtype == np.float64), len(out_slot),
                       len(site_lines) if n_entries is None else n_entries, n_out)
    return b''.join([head, np.asarray(tensor_row, dtype=np.int32).tobytes(), np.asarray(prob_row, dtype=np.int32).tobytes(), tensors.tobytes(), probs.tobytes(),
                     np.asarray(site_off, dtype=np.int64).tobytes(), np.asarray(site_lines, dtype=np.int32).tobytes(), np.asarray(out_slot, dtype=np.int32).tobytes()])


def run_host(exe, tmp_path, blob):
    """-> (the process, None) or (the process, (bad_site, (n, 1056) int32, (n, 90) float32, (n, 90) int64))"""
    case, res = os.path.join(str(tmp_path), 'case.bin'), os.path.join(str(tmp_path), 'result.bin')
    with open(case, 'wb') as f:
        f.write(blob)
    p = subprocess.run([exe, case, res], capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        return p, None
    raw = open(res, 'rb').read()
    bad, n = struct.unpack('<2q', raw[:16])
    a, b = 16 + n * CELLS * 4, 16 + n * CELLS * 4 + n * PROBS * 4
    return p, (bad, np.frombuffer(raw[16:a], dtype=np.int32).reshape(n, CELLS), np.frombuffer(raw[a:b], dtype=np.float32).reshape(n, PROBS),
               np.frombuffer(raw[b:], dtype=np.int64).reshape(n, PROBS))


def parse_lines(text):
    """the lines of --output_for_ensemble -> (keys, reference strings, (n, 1056) int32, (n, 90) float64)"""
    keys, seqs, cells, probs = [], [], [], []
    for row in text.splitlines():
        f = row.split('\t')
        assert len(f) == 3 + CELLS + PROBS
        keys.append((f[0], f[1]))
        seqs.append(f[2])
        cells.append([int(v) for v in f[3:3 + CELLS]])
        probs.append([float(v) for v in f[3 + CELLS:]])
    return keys, seqs, np.array(cells, dtype=np.int32).reshape(-1, CELLS), np.array(probs, dtype=np.float64).reshape(-1, PROBS)


def micro_text(m, negative_zero):
    if m == 0:
        return '-0.000000' if negative_zero else '0.000000'
    return '%s%d.%06d' % ('-' if m < 0 else '', abs(m) // 1000000, abs(m) % 1000000)


def host_ensemble_text(exe, tmp_path, text, minimum_count):
    """ensemble.py's output through the host build: its micro-units formatted, and the float32 alone printed '%.6f'"""
    keys, seqs, cells, probs = parse_lines(text)
    site_off, site_lines, out_slot, n_out, first = grouping(keys, minimum_count)
    rows = list(range(len(keys)))
    p, got = run_host(exe, tmp_path, case_bytes(rows, rows, cells, probs, site_off, site_lines, out_slot, n_out))
    assert p.returncode == 0, p.stderr[-2000:]
    bad, out_t, out_p, out_m = got
    assert bad == -1
    exact, through_float32 = [], []
    for s, slot in enumerate(out_slot):
        if slot < 0:
            continue
        head = [keys[first[s]][0], keys[first[s]][1], seqs[first[s]]] + [str(v) for v in out_t[slot].tolist()]
        exact.append('\t'.join(head + [micro_text(m, z) for m, z in zip(out_m[slot].tolist(), np.signbit(out_p[slot]).tolist())]) + '\n')
        through_float32.append('\t'.join(head + ['%.6f' % v for v in out_p[slot].tolist()]) + '\n')
    return ''.join(exact), ''.join(through_float32)


def random_blocks(seed, n_t, n_p, f64=False):
    """tensors with cells of either sign and probabilities as a network gives them (float32) or a text tool parses them (float64)"""
    rng = np.random.default_rng(seed)
    tensors = rng.integers(-50, 200, size=(n_t, CELLS), dtype=np.int32)
    probs = rng.random((n_p, PROBS), dtype=np.float32)
    probs[rng.random((n_p, PROBS)) < 0.2] = 0
    probs[rng.random((n_p, PROBS)) < 0.05] = 1
    if f64:
        probs = (np.rint(probs.astype(np.float64) * 1e6) / 1e6) + np.where(rng.random((n_p, PROBS)) < 0.1, 1 / 256, 0)
    return tensors, probs
