"""CPU test: one forward pass of Clair's network through the arithmetic and the index maps the kernels use (csrc/clair_net_core.h),
built for the host with g++ (scripts/clair_net_host_check.cpp, under AddressSanitizer and UBSan where the toolchain has their
runtimes), equals the restatement (tests/clair_net_ref.py) within the accuracy rule of the GPU test: its largest deviation from the
float64 values is at most 4 x that of the restatement in float32 -- before any of it meets a GPU."""
import os
import subprocess

import numpy as np
import pytest

import clair_net_ref as ref
from megapath_nano_amd import clair_net as cn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (('lstm1', 33 * 256), ('lstm2', 33 * 256), ('l3', 7680), ('l4', 192), ('probs', 90))


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp('clair_net_host') / 'clair_net_host_check'
    src = os.path.join(ROOT, 'scripts', 'clair_net_host_check.cpp')
    base = ['g++', '-std=c++17', '-Wall', '-Werror', '-o', str(out), src]
    if subprocess.run(base + ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']).returncode != 0:
        subprocess.run(base + ['-O2'], check=True)
    return out


def run(exe, tmp_path, weights, tensors):
    wf, tf, rf = tmp_path / 'weights.bin', tmp_path / 'tensors.bin', tmp_path / 'results.bin'
    cn.pack_weights(weights).tofile(wf)
    with open(tf, 'wb') as f:
        f.write(np.uint32(len(tensors)).tobytes() + np.ascontiguousarray(tensors, dtype='<i4').tobytes())
    subprocess.run([str(exe), str(wf), str(tf), str(rf)], check=True, timeout=600)
    flat = np.fromfile(rf, dtype='<f4').reshape(len(tensors), -1)
    assert flat.shape[1] == sum(s for _, s in SIZES)
    out, at = {}, 0
    for name, size in SIZES:
        out[name] = flat[:, at:at + size]
        at += size
    return out


@pytest.mark.parametrize('family', ['counts', 'small'])
def test_host_build_equals_the_restatement(exe, tmp_path, family):
    weights = ref.seeded_weights(11)
    tensors = ref.counts_inputs(6, 21) if family == 'counts' else ref.small_inputs(6, 22)
    p64, t64, dev = ref.deviations(weights, tensors)
    got = run(exe, tmp_path, weights, tensors)
    want = dict(t64, probs=p64)
    for name, _ in SIZES:
        ok, d = ref.within(got[name], want[name].reshape(len(tensors), -1), dev[name])
        print(f'{family} {name}: host build {d:.3e}, float32 restatement {dev[name]:.3e}')
        assert ok, (name, d, dev[name])
    assert np.abs(got['probs'].reshape(len(tensors), -1).sum(axis=1) - 4).max() < 1e-5


def test_host_build_refuses_a_short_weight_file(exe, tmp_path):
    (tmp_path / 'w.bin').write_bytes(b'\0' * 64)
    (tmp_path / 't.bin').write_bytes(np.uint32(0).tobytes())
    assert subprocess.run([str(exe), str(tmp_path / 'w.bin'), str(tmp_path / 't.bin'), str(tmp_path / 'r.bin')], stderr=subprocess.DEVNULL).returncode == 2
