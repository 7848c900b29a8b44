"""CPU test: the averaging through the arithmetic and the checks the kernel uses (csrc/clair_ensemble_core.h), built for the host
with g++ under AddressSanitizer and UBSan (scripts/clair_ensemble_host_check.cpp), reproduces what the reference's own ensemble.py
printed -- before any of it meets a GPU --, refuses malformed lists, and rounds exactly as `%.6f` does."""
import numpy as np
import pytest

import clair_ensemble_cases as ec
from megapath_nano_amd import clair_ensemble


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return ec.build_host_check(tmp_path_factory.mktemp('clair_ensemble_host'))


@pytest.mark.parametrize('name', ec.ENSEMBLE_NAMES)
def test_host_build_on_the_goldens(exe, tmp_path, name):
    """the micro-units reproduce the script's text everywhere; the float32 alone, printed '%.6f', does so for every value below 8
    (a float32 keeps six decimals only there), which is why the text tool formats the micro-units"""
    case = ec.ensemble_case(name)
    exact, through_float32 = ec.host_ensemble_text(exe, tmp_path, case['input'], case['minimum_count'])
    assert exact == case['output']
    if name == 'wide_values':
        assert through_float32 != case['output']
    else:
        assert through_float32 == case['output']


def test_the_rounding_equals_printf_everywhere(exe):
    """every s / c for s in 0 .. 2 000 000 and c in {1, 2, 3, 4, 7, 100, 400}, every tie j / 128 below 8 and both float64 neighbours of
    each: zero exceptions"""
    import subprocess
    p = subprocess.run([exe, '--rounding'], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout, p.stderr[-2000:])
    cases, wrong = (int(v) for v in p.stdout.split())
    assert wrong == 0 and cases == 7 * 2000001 + 512 * 6 + 12


def small(n_lines=6):
    tensors, probs = ec.random_blocks(3, 4, 5)
    return dict(tensor_row=[i % 4 for i in range(n_lines)], prob_row=[i % 5 for i in range(n_lines)], tensors=tensors, probs=probs,
                site_off=[0, 2, 3, 6], site_lines=[0, 3, 1, 2, 4, 5], out_slot=[0, -1, 1], n_out=2)


def test_shared_rows_float64_and_the_overflow_status(exe, tmp_path):
    case = small()
    p, got = ec.run_host(exe, tmp_path, ec.case_bytes(**case))
    assert p.returncode == 0, p.stderr
    bad, out_t, out_p, out_m = got
    t, pr = case['tensors'].astype(np.int64), case['probs']
    assert bad == -1 and (out_t[0] == t[0] + t[3]).all() and (out_t[1] == t[2] + t[0] + t[1]).all()
    quantized = np.rint(pr.astype(np.float64) * 1e6) / 1e6
    want = (quantized[0] + quantized[3]) / 2
    assert np.abs(out_p[0] - want).max() < 1e-6 and (np.abs(out_m[0] - want * 1e6) <= 0.5000001).all()
    f64 = dict(case, probs=quantized)
    p, again = ec.run_host(exe, tmp_path, ec.case_bytes(**f64))
    assert again[2].tobytes() == out_p.tobytes() and again[3].tobytes() == out_m.tobytes()          # float32 lines add what their text would
    big = dict(case, tensors=np.where(np.arange(4)[:, None] == 2, np.int32(2 ** 30), case['tensors']).astype(np.int32), tensor_row=[0, 1, 2, 3, 2, 2])
    p, got = ec.run_host(exe, tmp_path, ec.case_bytes(**big))
    assert p.returncode == 0 and got[0] == 2          # site 2 holds lines 2, 4, 5: three times 2^30


def test_malformed_lists_are_refused(exe, tmp_path):
    case = small()
    for change in (dict(tensor_row=[0, 1, 2, 4, 0, 1]), dict(prob_row=[0, 1, 2, -1, 0, 1]), dict(site_lines=[0, 3, 1, 2, 4, 6]), dict(site_lines=[0, 3, 1, 2, 4, -1]),
                   dict(site_off=[0, 2, 2, 6]), dict(site_off=[0, 2, 3, 7]), dict(site_off=[1, 2, 3, 6]), dict(site_off=[0, 4, 3, 6]), dict(out_slot=[0, -1, 0]),
                   dict(out_slot=[0, -1, 2]), dict(out_slot=[0, -2, 1]), dict(out_slot=[0, -1, -1]), dict(n_out=4), dict(n_out=1)):
        p, got = ec.run_host(exe, tmp_path, ec.case_bytes(**dict(case, **change)))
        assert p.returncode == 3 and got is None and 'refused' in p.stderr, (change, p.returncode, p.stderr)
    p, _ = ec.run_host(exe, tmp_path, ec.case_bytes(**case)[:200])
    assert p.returncode == 2


def test_the_grouping_of_the_python_layer():
    """clair_ensemble.group equals the dictionary walk, for strings and for an integer array"""
    import random
    rng = random.Random(6)
    keys = [('c', str(rng.randrange(30))) for _ in range(400)]
    for m in (0, 1, 12, 20):
        want = ec.grouping(keys, m)
        for got in (clair_ensemble.group(keys, m), clair_ensemble.group(np.array([int(k[1]) for k in keys]), m)):
            assert [got[0].tolist(), got[1].tolist(), got[2].tolist(), got[3]] == list(want[:4])
    empty = clair_ensemble.group([], 0)
    assert empty[0].tolist() == [0] and len(empty[1]) == 0 and len(empty[2]) == 0 and empty[3] == 0
