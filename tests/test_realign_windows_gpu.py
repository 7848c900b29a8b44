"""realigner.realign_windows on the GPU: consensus, the script's cut to 200 haplotypes, its skip rule and realign_batch, against
oracle.realign_oracle fed with the haplotypes of the restatement tests/dbg_ref.py."""
import pytest

import dbg_cases as dc
import dbg_ref
from megapath_nano_amd import realigner
from oracle import realign_oracle

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('libmpn')]


def make_window(seed, alt, ref_start):
    """a window of 60 bases between 50-base flanks; 8 reads of 70 bases, every other one from `alt`, all with a plain match CIGAR"""
    pre, suf = dc.rnd(50, seed), dc.rnd(50, seed + 1)
    full_ref, full_alt = pre + dc.R60 + suf, pre + alt + suf
    seqs, positions = [], []
    for i in range(8):
        src = full_alt if i % 2 else full_ref
        at = 20 + 5 * i
        seqs.append(src[at:at + 70])
        positions.append(ref_start + at)
    return dict(ref=dc.R60, graph_reads=seqs, graph_bad=[{3} if i == 2 else None for i in range(8)], ref_prefix=pre, ref_suffix=suf,
                seqs=seqs, positions=positions, cigars=['70M'] * 8, ref_start=ref_start)


def oracle_window(w):
    haps = dbg_ref.get_consensus(w['ref'], w['graph_reads'], [b or () for b in w['graph_bad']])[0][:200]
    if not haps or haps == [w['ref']] or not w['seqs']:
        return None
    return [tuple(x) for x in realign_oracle.realign_reads(
        w['seqs'], w['positions'], w['cigars'], w['ref_prefix'] + w['ref'] + w['ref_suffix'],
        [w['ref_prefix'] + h + w['ref_suffix'] for h in haps], w['ref_start'], len(w['ref_prefix']), len(w['ref_suffix']))]


def test_three_windows_equal_the_oracle_on_the_restatements_haplotypes():
    dele = dc.R60[:28] + dc.R60[31:]
    windows = [make_window(40, dc.S30, 1000), make_window(42, dc.R60, 5000), make_window(44, dele, 70)]
    want = [oracle_window(w) for w in windows]
    assert want[1] is None and want[0] is not None and want[2] is not None      # the middle window's consensus is its reference alone
    got = realigner.realign_windows(windows)
    assert [None if g is None else [tuple(x) for x in g] for g in got] == want
    assert any('D' in c for _, c in want[2])                                     # the deletion does reach the CIGARs
