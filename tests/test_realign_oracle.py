"""f4 oracle: the Python restatement of realigner.cpp (oracle/realign_oracle.py) against the golden vectors produced by the
reference's own sources compiled in place, and against that build's outputs on random windows."""
import json
import os

import numpy as np
import pytest

from oracle import realign_oracle as ro
from realign_cases import make_window, random_window_kwargs

pytestmark = pytest.mark.usefixtures('oracle_built')
GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'realign_golden.json')
GOLD_RANDOM = os.path.join(os.path.dirname(__file__), 'golden', 'realign_random_golden.json')
KEYS = ('seqs', 'positions', 'cigars', 'reference', 'haplotypes', 'ref_start', 'ref_prefix', 'ref_suffix')


def test_oracle_matches_golden():
    cases = json.load(open(GOLD))
    assert len(cases) >= 15
    n = 0
    for c in cases:
        got = ro.realign_reads(**{k: c[k] for k in KEYS})
        assert [list(x) for x in got] == c['expected']
        n += len(got)
    assert n > 600


def test_golden_covers_the_paths():
    """the fixtures exercise the fast (k-mer + Hamming) path, the SSW path, untouched reads and clipped results"""
    cases = json.load(open(GOLD))
    flat = [(e, p, c) for cs in cases for e, p, c in zip(cs['expected'], cs['positions'], cs['cigars'])]
    kinds = {''.join(ch for ch in e[1] if not ch.isdigit()) for e, _, _ in flat}
    assert {'X', 'XDX', 'XIX'} <= kinds and any('S' in k for k in kinds)
    assert any(e == [p, c] for e, p, c in flat)          # a read the realigner leaves alone
    assert any(len(cs['haplotypes']) > 16 for cs in cases)   # std::sort leaves its insertion-sort regime


def test_libstdcxx_sort_is_a_permutation_and_sorted():
    rng = np.random.default_rng(3)
    for n in (0, 1, 2, 15, 16, 17, 40, 200):
        keys = [int(x) for x in rng.integers(0, 5, n)]
        perm = ro.libstdcxx_sort(keys)
        assert sorted(perm) == list(range(n))
        assert [keys[i] for i in perm] == sorted(keys)
        if n <= 16:   # insertion sort only: stable
            assert perm == sorted(range(n), key=lambda i: keys[i])


def test_oracle_matches_compiled_reference_on_random_windows():
    """the compiled reference's outputs on these windows are stored in golden/realign_random_golden.json
    (golden/make_realign_golden.py)"""
    expected = json.load(open(GOLD_RANDOM))['expected']
    kws = random_window_kwargs()
    assert len(expected) == len(kws)
    for k, (kw, want) in enumerate(zip(kws, expected)):
        c = make_window(5000 + k, **kw)
        assert [list(x) for x in ro.realign_reads(**c)] == want, kw
