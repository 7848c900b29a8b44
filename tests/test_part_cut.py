"""CPU test: aligner.iter_target_parts_by_length (the part rule over (name, length), for targets whose bases are in HBM) cuts every
sequence of lengths exactly as aligner.iter_target_parts cuts the records; and the knob that chooses the path refuses unknown values."""
import numpy as np
import pytest

from megapath_nano_amd import aligner


def cuts_by_records(lens, batch_bases):
    recs = [(f'r{k}', b'A' * n) for k, n in enumerate(lens)]
    return [[(name, len(seq)) for name, seq in part] for part in aligner.iter_target_parts(iter(recs), batch_bases)]


def cuts_by_length(lens, batch_bases):
    recs = [(f'r{k}', n, 'payload') for k, n in enumerate(lens)]
    return [[(r[0], r[1]) for r in part] for part in aligner.iter_target_parts_by_length(iter(recs), batch_bases)]


@pytest.mark.parametrize('mini', [1, 50, 700, 10_000])
def test_length_cutter_agrees_with_record_cutter(monkeypatch, mini):
    monkeypatch.setattr(aligner, 'IDX_MINI_BATCH', mini)
    rng = np.random.default_rng(mini)
    n_lists = 0
    for _ in range(80):
        n = int(rng.integers(0, 40))
        lens = rng.integers(0, 400, size=n).tolist()
        for k in range(n):      # zero-length records, and records larger than every batch_bases below
            if rng.random() < 0.15:
                lens[k] = 0
            elif rng.random() < 0.05:
                lens[k] = int(rng.integers(3000, 6000))
        for batch_bases in (0, 1, 399, 1000, 2500, 10**9):
            want = cuts_by_records(lens, batch_bases)
            assert cuts_by_length(lens, batch_bases) == want
            assert [r for part in want for r in part] == [(f'r{k}', x) for k, x in enumerate(lens)]
            n_lists += 1
    assert n_lists == 480


def test_hand_worked_cut(monkeypatch):
    """mini-batch 100, batch 250: mini-batches close after 60+50 (110), 300 (410 > 250: part), 0+100 (100), 99+1 (200), 200 (400 > 250: part)"""
    monkeypatch.setattr(aligner, 'IDX_MINI_BATCH', 100)
    parts = cuts_by_length([60, 50, 300, 0, 100, 99, 1, 200, 7], 250)
    assert [[n for _, n in p] for p in parts] == [[60, 50, 300], [0, 100, 99, 1, 200], [7]]


def test_knob_values(monkeypatch):
    from megapath_nano_amd import ingest
    monkeypatch.delenv('MPN_TARGET_INGEST', raising=False)
    assert ingest.ingest_mode() == 'host' and not aligner.target_ingest_on_device(['/nonexistent.fna.gz'])
    monkeypatch.setenv('MPN_TARGET_INGEST', 'host')
    assert ingest.ingest_mode() == 'host'
    monkeypatch.setenv('MPN_TARGET_INGEST', 'device')
    assert ingest.ingest_mode() == 'device' and not aligner.target_ingest_on_device(['/nonexistent.fna.gz'])
    monkeypatch.setenv('MPN_TARGET_INGEST', 'gpu')
    with pytest.raises(ValueError):
        aligner.target_ingest_on_device(['x'])
