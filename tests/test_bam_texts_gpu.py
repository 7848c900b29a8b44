"""GPU tests (-m gpu) of ingest.BamTexts on its own, the iterator every reader of a BAM file stands on: the texts and their record
tables against the restatement tests/bam_in_ref.py on the files of tests/bam_in_cases.py -- plain iteration, texts that begin again
at an earlier record (keep_from), the absolute offset in the error for malformed text after such a restart, laziness, and what is
booked."""
import numpy as np
import pytest

import bam_in_cases as bc
import bam_in_ref as ref

pytestmark = pytest.mark.gpu
FIELDS = ('l_seq', 'flag', 'l_read_name', 'has_qual')


@pytest.fixture(scope='module')
def cases(libmpn, tmp_path_factory):
    """name -> dict(path, text, want): the files of bam_in_cases, walked once by the restatement"""
    d = tmp_path_factory.mktemp('bam_texts')
    out = {}
    for name, f in bc.files().items():
        p = d / f'{name}.bam'
        p.write_bytes(f['blob'])
        out[name] = dict(path=str(p), text=f['text'], want=[(r['off'],) + tuple(r[k] for k in FIELDS) for r in ref.walk(f['text'])])
    return out


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    monkeypatch.delenv('MPN_INGEST_BATCH_BYTES', raising=False)
    monkeypatch.delenv('MPN_BAM_WALK_RECORDS', raising=False)


def absolute(t):
    """the rows of a text with their offsets in the whole inflated stream"""
    return [(t.base + int(r['off']),) + tuple(int(r[k]) for k in FIELDS) for r in t.rows]


def assert_rows_point_at_their_records(t, whole):
    """the first and the last row of a text: block_size, the fixed fields and the name, in the text and in the whole stream"""
    assert 0 <= t.text_len <= t.text.numel() and t.base + t.text_len <= len(whole)
    for r in t.rows[[0, -1]] if len(t.rows) else ():
        a, n = int(r['off']), 36 + int(r['l_read_name'])
        assert t.text[a:a + n].cpu().numpy().tobytes() == whole[t.base + a:t.base + a + n]


@pytest.mark.parametrize('group,walk', [(None, None), (1 << 17, 3), (1, 1), (1, 64)])
@pytest.mark.parametrize('name', ['main', 'cuts', 'no_eof', 'stored', 'header_only', 'only_empty_reads'])
def test_plain_iteration_gives_every_record_once(cases, monkeypatch, name, group, walk):
    from megapath_nano_amd import ingest
    if group is not None:
        monkeypatch.setenv('MPN_INGEST_BATCH_BYTES', str(group))
    c = cases[name]
    got, finals = [], []
    with ingest.BamTexts(c['path'], walk_records=walk) as texts:
        for t in texts:
            assert t.rows.dtype == ingest.BAM_ROW
            got += absolute(t)
            finals.append(t.final)
            assert_rows_point_at_their_records(t, c['text'])
    assert got == c['want']
    assert finals == [False] * (len(finals) - 1) + [True]
    if group == 1 << 17 and name == 'main':
        assert len(finals) > 2


@pytest.mark.parametrize('where', ['first', 'middle', 'behind_the_last'])
def test_a_text_begins_at_the_record_that_was_kept(cases, monkeypatch, where):
    from megapath_nano_amd import ingest
    monkeypatch.setenv('MPN_INGEST_BATCH_BYTES', str(1 << 17))
    c = cases['main']
    seen, expect, n_texts = [], None, 0
    with ingest.BamTexts(c['path'], walk_records=5) as texts:
        for t in texts:
            rows = absolute(t)
            if expect is not None:
                assert rows[:len(expect)] == expect            # the same absolute offsets, l_seq and flags again
            assert_rows_point_at_their_records(t, c['text'])
            seen += rows
            n_texts += 1
            if not t.final:
                k = {'first': 0, 'middle': len(rows) // 2, 'behind_the_last': len(rows)}[where]
                for bad in (len(rows) + 1, -1):
                    with pytest.raises(ValueError, match='keep_from'):
                        texts.keep_from(bad)
                texts.keep_from(k)
                expect = rows[k:]
    assert n_texts > 2
    assert sorted(set(seen)) == c['want']
    if where == 'behind_the_last':
        assert seen == c['want']


def test_the_offset_of_malformed_text_is_absolute_after_a_restart(libmpn, tmp_path, monkeypatch):
    """every text restarts at the last record of the one before, so base is not the sum of the walks' ends"""
    from megapath_nano_amd import ingest
    monkeypatch.setenv('MPN_INGEST_BATCH_BYTES', '64')
    for name, text, status, offset, n in bc.malformed_texts():
        p = tmp_path / f'{name}.bam'
        p.write_bytes(bc.bgzf(text, cuts=range(0, len(text), 50)))
        seen = set()
        with pytest.raises(ValueError, match=f'offset {offset} of the inflated stream: {ingest.STATUS_NAMES[status]}$') as e:
            with ingest.BamTexts(str(p)) as texts:
                for t in texts:
                    seen |= {t.base + int(off) for off in t.rows['off']}
                    texts.keep_from(max(len(t.rows) - 1, 0))
        assert str(e.value).startswith(f'{p}: BAM text at offset ') and len(seen) <= n, name


def test_nothing_is_read_before_the_first_text(libmpn, tmp_path):
    from megapath_nano_amd import ingest
    p = tmp_path / 'no.bam'
    p.write_bytes(b'this is not a BAM file')
    for path in (str(p), str(tmp_path / 'missing.bam')):
        with ingest.BamTexts(path) as texts:
            assert iter(texts) is texts
    with pytest.raises(ValueError, match='not a BGZF block at file offset 0'):
        with ingest.BamTexts(str(p)) as texts:
            next(texts)


def test_a_stream_of_the_caller_is_left_open(cases):
    from megapath_nano_amd import ingest
    c = cases['only_empty_reads']
    with open(c['path'], 'rb') as stream:
        with ingest.BamTexts(stream) as texts:
            got = [row for t in texts for row in absolute(t)]
        assert got == c['want'] and not stream.closed and stream.read() == b''


def test_the_walk_is_booked_and_records_are_not(cases):
    from megapath_nano_amd import ingest
    c = cases['main']
    for w in (7, len(c['want'])):
        timings = {}
        with ingest.BamTexts(c['path'], timings=timings, walk_records=w) as texts:
            assert sum(len(t.rows) for t in texts) == len(c['want'])
        assert timings['walk_launches'] == len(c['want']) // w + 1
        assert timings['walk_device_ms'] > 0 and timings['walk'] > 0 and 'records' not in timings
        assert {'read', 'h2d', 'inflate', 'flatten'} <= set(timings)
