"""GPU tests (-m gpu) of the averaging of Clair's lines per site (megapath_nano_amd/clair_ensemble.py, csrc/clair_ensemble_kernels.hip):
the device equals the host build of the same arithmetic (scripts/clair_ensemble_host_check.cpp) exactly, on int32 values and on
float32 bit patterns, and the text tool prints what the reference's own ensemble.py printed, byte for byte."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import clair_ensemble_cases as ec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ens(libmpn):
    from megapath_nano_amd import clair_ensemble
    return clair_ensemble


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return ec.build_host_check(tmp_path_factory.mktemp('clair_ensemble_host'))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def lists_of(counts, n_t, n_p, seed, dropped=()):
    """sites of counts[s] lines whose lines are interleaved over the input, as resamples and models interleave them; tensor rows shared"""
    rng = np.random.default_rng(seed)
    site = rng.permutation(np.repeat(np.arange(len(counts)), counts))
    n = len(site)
    tensor_row, prob_row = rng.integers(0, n_t, n), rng.permutation(n_p)[:n] if n_p >= n else rng.integers(0, n_p, n)
    site_lines = np.argsort(site, kind='stable')
    site_off = np.concatenate([[0], np.cumsum(counts)])
    out_slot, k = [], 0
    for s in range(len(counts)):
        out_slot.append(-1 if s in dropped else k)
        k += s not in dropped
    return dict(tensor_row=tensor_row, prob_row=prob_row, site_off=site_off, site_lines=site_lines, out_slot=out_slot, n_out=k)


def both(ens, exe, tmp_path, lists, tensors, probs):
    """-> (device, host): bad site, int32 sums, float32 means, int64 micro-units"""
    p, host = ec.run_host(exe, tmp_path, ec.case_bytes(tensors=tensors, probs=probs, **lists))
    assert p.returncode == 0, p.stderr[-2000:]
    out_t, out_p, out_m, bad = ens.ensemble_rows(lists['tensor_row'], lists['prob_row'], dev(tensors).reshape(-1), dev(probs), lists['site_off'], lists['site_lines'],
                                                 lists['out_slot'], lists['n_out'], micro=True)
    return (bad, out_t.cpu().numpy(), out_p.cpu().numpy(), out_m.cpu().numpy()), host


def same(got, want):
    assert got[0] == want[0] == -1
    assert got[1].shape == want[1].shape and got[1].tobytes() == want[1].tobytes()
    assert got[2].tobytes() == want[2].tobytes()                   # float32 bit patterns
    assert got[3].tobytes() == want[3].tobytes()


@pytest.mark.parametrize('f64', [False, True])
def test_sites_of_many_depths_in_one_call(ens, exe, tmp_path, f64):
    """1, 2, 63, 64, 65, 100 and 401 lines: below, at and above the unrolled step of 8 and a wave's 64; float32 and float64 input"""
    counts = [1, 2, 63, 64, 65, 100, 401, 7, 8, 9]
    tensors, probs = ec.random_blocks(21, 300, sum(counts), f64)
    lists = lists_of(counts, 300, sum(counts), 5)
    got, want = both(ens, exe, tmp_path, lists, tensors, probs)
    same(got, want)
    again, _ = both(ens, exe, tmp_path, lists, tensors, probs)
    same(again, want)                                              # the same from run to run


def test_5000_shallow_sites_next_to_a_deep_one(ens, exe, tmp_path):
    counts = [1] * 2500 + [401] + [1] * 2500
    tensors, probs = ec.random_blocks(22, 500, 600)
    got, want = both(ens, exe, tmp_path, lists_of(counts, 500, 600, 6), tensors, probs)
    same(got, want)


def test_one_site_alone_and_no_lines(ens, exe, tmp_path):
    tensors, probs = ec.random_blocks(23, 3, 3)
    for counts in ([1], [3]):
        got, want = both(ens, exe, tmp_path, lists_of(counts, 3, 3, 7), tensors, probs)
        same(got, want)
    import torch
    empty_t, empty_p = torch.zeros(0, dtype=torch.int32, device='cuda'), torch.zeros((0, 90), dtype=torch.float32, device='cuda')
    for t, p in ((empty_t, empty_p), (dev(tensors).reshape(-1), dev(probs))):
        out_t, out_p, out_m, bad = ens.ensemble_rows([], [], t, p, [0], [], [], 0, micro=True)
        assert tuple(out_t.shape) == (0, 1056) and tuple(out_p.shape) == (0, 90) and bad == -1
    sites, sums, means = ens.ensemble([], empty_t.reshape(0, 33, 8, 4), [empty_p, empty_p], minimum_count=2)
    assert sites == [] and tuple(sums.shape) == (0, 33, 8, 4) and tuple(means.shape) == (0, 90)


def test_dropped_sites_first_last_and_every_second(ens, exe, tmp_path):
    counts = [3, 1, 2, 1, 9, 1, 2, 1, 5]
    tensors, probs = ec.random_blocks(24, 10, 40)
    for dropped in ((0,), (8,), (0, 8), (1, 3, 5, 7), (0, 2, 4, 6, 8), tuple(range(9))):
        got, want = both(ens, exe, tmp_path, lists_of(counts, 10, 40, 8, dropped), tensors, probs)
        same(got, want)
        assert len(got[1]) == 9 - len(dropped)


def test_three_models_over_shared_tensors(ens, exe, tmp_path):
    """ensemble(): one tensor block, three probability blocks; a site's lines lie in all three and its tensor rows are named three
    times; positions repeat inside a model (resamples); minimum_count drops the position that only one line names"""
    import torch
    centres =[500, 17, 500, 42, 17, 500, 9, 10, 42]
    n = len(centres)
    tensors, probs = ec.random_blocks(25, n, 3 * n)
    for minimum_count in (0, 4, 7):
        sites, sums, means = ens.ensemble(centres, dev(tensors).reshape(n, 33, 8, 4), [dev(probs[k * n:(k + 1) * n]) for k in range(3)], 'ctg', minimum_count)
        keys = centres * 3
        site_off, site_lines, out_slot, n_out, first = ec.grouping(keys, minimum_count)
        p, want = ec.run_host(exe, tmp_path, ec.case_bytes([i % n for i in range(3 * n)], list(range(3 * n)), tensors, probs, site_off, site_lines, out_slot, n_out))
        assert p.returncode == 0, p.stderr
        assert sites == [keys[f] for f, s in zip(first, out_slot) if s >= 0] and len(sites) == {0: 5, 4: 3, 7: 1}[minimum_count]
        assert sums.dtype == torch.int32 and tuple(sums.shape) == (n_out, 33, 8, 4) and sums.cpu().numpy().tobytes() == want[1].tobytes()
        assert means.cpu().numpy().tobytes() == want[2].tobytes()
    # K pairs: every model with its own tensors and centres
    pairs = ens.ensemble([centres[:4], centres[4:]], [dev(tensors[:4]), dev(tensors[4:])], [dev(probs[:4]), dev(probs[4:n])])
    whole = ens.ensemble(centres, dev(tensors), [dev(probs[:n])])
    assert pairs[0] == whole[0] and torch.equal(pairs[1], whole[1]) and torch.equal(pairs[2], whole[2])


def test_the_overflow_status_and_refusals(ens, exe, tmp_path):
    tensors, probs = ec.random_blocks(26, 4, 8)
    tensors[1, 700] = tensors[2, 700] = 2 ** 30
    tensors[3, 5] = -2 ** 31
    lists = dict(tensor_row=[0, 1, 2, 3, 3, 1, 2, 0], prob_row=list(range(8)), site_off=[0, 2, 4, 6, 8], site_lines=[0, 1, 2, 7, 3, 4, 5, 6], out_slot=[0, 1, 2, 3], n_out=4)
    p, host = ec.run_host(exe, tmp_path, ec.case_bytes(tensors=tensors, probs=probs, **lists))
    out = ens.ensemble_rows(lists['tensor_row'], lists['prob_row'], dev(tensors).reshape(-1), dev(probs), lists['site_off'], lists['site_lines'], lists['out_slot'], 4)
    assert out[3] == host[0] == 2                 # site 2 = lines 3, 4: twice -2^31; site 3 = lines 5, 6: 2^30 + 2^30; the smallest is reported
    with pytest.raises(ValueError, match='ctg:7: a sum'):
        ens.ensemble([5, 7, 7, 6], dev(tensors), [dev(probs[:4])], 'ctg')          # rows 1 and 2: 2^30 + 2^30
    t, pr = dev(tensors).reshape(-1), dev(probs)
    for change in (dict(tensor_row=[0, 1, 2, 4, 3, 1, 2, 0]), dict(prob_row=[0, 1, 2, 3, 4, 5, 6, 8]), dict(site_lines=[0, 1, 2, 7, 3, 4, 5, 8]),
                   dict(site_off=[0, 2, 2, 6, 8]), dict(out_slot=[0, 1, 1, 2]), dict(out_slot=[0, 1, 2, 4]), dict(out_slot=[0, -1, 1, 2])):
        bad = dict(lists, **change)
        with pytest.raises(ValueError):
            ens.ensemble_rows(bad['tensor_row'], bad['prob_row'], t, pr, bad['site_off'], bad['site_lines'], bad['out_slot'], 4)
    for wrong_t, wrong_p in ((t.to(torch_dtype('int64')), pr), (t, pr.to(torch_dtype('float16'))), (t.cpu(), pr), (t, pr[:, :80]), (t[:-1], pr)):
        with pytest.raises(ValueError):
            ens.ensemble_rows(lists['tensor_row'], lists['prob_row'], wrong_t, wrong_p, lists['site_off'], lists['site_lines'], lists['out_slot'], 4)


def torch_dtype(name):
    import torch
    return getattr(torch, name)


@pytest.mark.parametrize('name', ec.ENSEMBLE_NAMES)
def test_the_golden_lines_through_ensemble_lines(ens, name):
    case = ec.ensemble_case(name)
    out = io.BytesIO()
    n = ens.ensemble_lines(io.StringIO(case['input']), out, case['minimum_count'])
    assert out.getvalue().decode() == case['output'] and n == case['output'].count('\n')


def test_the_tool_and_its_refusals(ens):
    case = ec.ensemble_case('thirds_and_sevenths')
    tool = os.path.join(ec.ROOT, 'bin', 'mpn-ensemble')
    p = subprocess.run([sys.executable, tool, '--minimum_count_to_output', '3'], input=case['input'].encode(), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert p.stdout.decode() == case['output']
    first = case['input'].splitlines(keepends=True)[0]
    for bad in (first.rstrip('\n') + '\t0.5\n', '\t'.join(first.split('\t')[:-1]) + '\n', first.replace('\t0\t', '\t3000000000\t', 1), first.rstrip('\n') + 'x\n',
                '\t'.join(first.split('\t')[:-1] + ['nan\n']), '\n'):
        with pytest.raises(ValueError, match='line 2'):
            ens.ensemble_lines(io.StringIO(first + bad), io.BytesIO())
