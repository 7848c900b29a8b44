"""The restatement of the FASTQ scan (tests/fastq_scan_ref.py) against fastx.iter_fastx, which defines the records: for every text
the device tests use, the accepted prefix reads as exactly the records iter_fastx yields for those bytes, and iter_fastx started at
`consumed` yields the rest of the file's records.  Runs without a GPU."""
import re

import pytest

import fastq_scan_ref as ref
from megapath_nano_amd import ingest

TILE = ref.header_tile()


def _check(text, final, want_n=None, want_status=None):
    rows, consumed, status = ref.scan(text, final)
    got = ref.records(text, rows)
    assert got == ref.host_records(text[:consumed])
    assert got + ref.host_records(text[consumed:]) == ref.host_records(text)
    # the rows lie inside the text, in order, and `consumed` is a line start
    assert 0 <= consumed <= len(text) and (consumed == 0 or consumed == len(text) or text[consumed - 1:consumed] == b'\n')
    for w in rows:
        assert 0 <= w['name_off'] <= w['seq_off'] <= w['seq_off'] + w['len'] <= w['qual_off'] <= w['qual_off'] + w['len'] <= consumed
    if want_n is not None:
        assert len(rows) == want_n
    if want_status is not None:
        assert status == want_status
    return rows, consumed, status


@pytest.mark.parametrize('case', ref.plain_cases(TILE), ids=lambda c: c[0])
def test_plain_texts(case):
    _, text, final = case
    rows, consumed, status = _check(text, final, want_status=ref.OK)
    if final:
        assert consumed == len(text) and len(rows) == len(ref.host_records(text))
    else:
        assert len(rows) == len(ref.host_records(text)) - (1 if consumed < len(text) else 0)


def test_edge_cases_put_line_starts_on_the_edges():
    seen = 0
    for name, text, _ in ref.plain_cases(TILE):
        m = re.fullmatch(r'edge(\d)_([+-]\d)_line(\d)', name)
        if m:
            w = ref.scan(text, True)[0][1]
            starts = (int(w['name_off']) - 1, int(w['seq_off']), int(w['seq_off']) + int(w['len']) + 1, int(w['qual_off']))
            assert starts[int(m.group(3))] == int(m.group(1)) * TILE + int(m.group(2))
            seen += 1
    assert seen == 2 * 5 * 4


@pytest.mark.parametrize('case', ref.cut_cases(), ids=lambda c: c[0])
def test_cuts_stop_at_the_record_start(case):
    _, text, cut = case
    whole, _, _ = ref.scan(text, True)
    rows, consumed, status = _check(text[:cut], False, want_status=ref.OK)
    ends = [0] + [int(w['qual_off']) + int(w['len']) + 1 for w in whole]
    assert consumed == max(e for e in ends if e <= cut)
    # resuming with the carried tail gives the rows of the uncut text
    rest, consumed2, status2 = ref.scan(text[consumed:], True)
    assert status2 == ref.OK and consumed + consumed2 == len(text)
    assert ref.records(text[:cut], rows) + ref.records(text[consumed:], rest) == ref.records(text, whole)


@pytest.mark.parametrize('case', ref.unsupported_cases(), ids=lambda c: c[0])
def test_unsupported_records_end_the_prefix(case):
    _, text, final, before = case
    rows, consumed, _ = _check(text, final, want_n=before, want_status=ref.UNSUPPORTED)
    assert consumed == sum(len(g) for g in ref.GOOD[:before])


def test_truncated_record_without_final_is_carried():
    for _, bad in ref.TRUNCATED:
        _check(ref.GOOD[0] + bad, False, want_n=1, want_status=ref.OK)


@pytest.mark.parametrize('case', ref.htslib_cases(), ids=lambda c: c[0])
def test_htslib_files(case):
    _, text, want = case
    rows, consumed, status = _check(text, True)
    if want is None:
        assert status == ref.OK and consumed == len(text) and len(rows) == len(ref.host_records(text)) > 0
    else:
        assert status == ref.UNSUPPORTED and len(rows) == want


def test_read_ingest_mode(monkeypatch):
    monkeypatch.delenv('MPN_READ_INGEST', raising=False)
    assert ingest.read_ingest_mode() == 'host'
    monkeypatch.setenv('MPN_READ_INGEST', 'device')
    assert ingest.read_ingest_mode() == 'device'
    monkeypatch.setenv('MPN_READ_INGEST', 'bogus')
    with pytest.raises(ValueError):
        ingest.read_ingest_mode()
