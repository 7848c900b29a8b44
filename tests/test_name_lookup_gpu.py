"""GPU tests (-m gpu) of mpn_name_set_create and mpn_fastq_name_lookup on their own: `found` against a Python dict on the name cases
of tests/name_cases.py, with the ids at every alignment of the text, at its first record and at its end, and with tables that are
nearly full.  The heads are written down from the texts' construction, so nothing but the lookup is under test."""
import numpy as np
import pytest

import name_cases

pytestmark = pytest.mark.gpu


def on_device(text):
    """-> (uint8 device tensor of the text and 16 bytes behind it, the text's length)"""
    import torch
    return torch.from_numpy(np.frombuffer(bytes(text) + b'\0' * 16, dtype=np.uint8).copy()).cuda(), len(text)


def text_of(ids, seq_len=lambda k: 3 + k % 5):
    """FASTQ records `@id[ c]` with short reads -> (text, heads); every third header has a comment"""
    from megapath_nano_amd import fastq_filter as ff
    parts, heads, at = [], np.zeros(len(ids), dtype=ff.FASTQ_HEAD), 0
    for k, x in enumerate(ids):
        n = seq_len(k)
        comment = b' c' if k % 3 == 0 else b''
        rec = b'@' + x + comment + b'\n' + b'A' * n + b'\n+\n' + b'I' * n + b'\n'
        heads[k] = (at + 1, len(x), len(comment) - 1 if comment else -1)
        parts.append(rec)
        at += len(rec)
    return b''.join(parts), heads


def lookup(text, heads, names, slots=0):
    from megapath_nano_amd import fastq_filter as ff
    d_text, n = on_device(text)
    with ff.NameSet(names, slots) as s:
        assert s.first_of.tolist() == name_cases.want_found(names, names)
        return ff.fastq_name_lookup(d_text, n, heads, s).tolist()


def ids_of(text, heads):
    return [text[int(h['off']):int(h['off']) + int(h['id_len'])] for h in heads]


@pytest.fixture(scope='module')
def all_ids():
    return name_cases.ids()


def test_every_id_at_every_alignment(libmpn, all_ids):
    """each id of the cases at every residue of its offset mod 16, against the whole list, half of it, and strangers"""
    queries = all_ids + [b'absent', all_ids[3] + b'!', all_ids[9][:-1], all_ids[10][:39]]
    while (len(queries) + 2) % 3:                    # a block is a filler, the queries and a trailer: the comments repeat with it
        queries.append(b'absent%d' % len(queries))
    blocks = []
    for shift in range(16):
        # every block starts at a multiple of 16: its filler moves the queries by `shift` bytes, its trailer fills the block up
        block = [b'p' * ((shift - 10) % 16)] + queries
        block.append(b't' * ((-len(text_of(block + [b''], seq_len=lambda k: 1)[0])) % 16))
        assert len(text_of(block, seq_len=lambda k: 1)[0]) % 16 == 0
        blocks += block
    text, heads = text_of(blocks, seq_len=lambda k: 1)
    for x in queries:
        offs = {int(h['off']) % 16 for h, y in zip(heads, blocks) if y == x}
        assert offs == set(range(16)), x[:20]
    assert ids_of(text, heads) == blocks
    for names in (all_ids, all_ids[::2], all_ids[::-1], all_ids + all_ids[::-1] + all_ids[:5]):
        assert lookup(text, heads, names) == name_cases.want_found(names, blocks)


def test_the_first_record_and_the_end_of_the_text(libmpn, all_ids):
    from megapath_nano_amd import fastq_filter as ff
    names = all_ids + [b'last']
    for x in all_ids:
        text, heads = text_of([x, b'mid', b'last'])
        assert heads['off'][0] == 1
        assert lookup(text, heads, names) == name_cases.want_found(names, [x, b'mid', b'last'])
    # The text ends at a multiple of 16, and one byte behind one.  The id of the last record lies as close to the end as a record
    # allows -- an empty read whose last line has no line feed: '@id' LF LF '+' LF -- and then in a whole last record whose quality
    # line, with its line feed, ends exactly at text_len.
    for over in (0, 1):
        for tail_id in (b'last', all_ids[2], all_ids[4], all_ids[7]):
            for tail in (b'\n\n+\n', b'\nACGT\n+\nIIII\n'):
                last = b'@' + tail_id + tail
                fill = (over - len(b'@f\n\n+\n\n') - len(last)) % 16
                first_id = b'f' + b'x' * fill
                text = b'@' + first_id + b'\n\n+\n\n' + last
                assert len(text) % 16 == over
                heads = np.zeros(2, dtype=ff.FASTQ_HEAD)
                heads[0] = (1, len(first_id), -1)
                heads[1] = (len(text) - len(last) + 1, len(tail_id), -1)
                assert ids_of(text, heads) == [first_id, tail_id]
                assert lookup(text, heads, names) == name_cases.want_found(names, [first_id, tail_id])


def test_lists_empty_single_and_either_side_of_a_doubling(libmpn, all_ids):
    from megapath_nano_amd import fastq_filter as ff
    queries = all_ids[:12] + [b'n%d' % i for i in range(10)] + [b'one']
    text, heads = text_of(queries)
    assert lookup(text, heads, []) == [-1] * len(queries)
    assert lookup(text, heads, [b'one']) == name_cases.want_found([b'one'], queries)
    assert lookup(text, heads, [b'']) == name_cases.want_found([b''], queries)
    for k in (8, 9):
        names = [b'n%d' % i for i in range(k)]
        assert lookup(text, heads, names) == name_cases.want_found(names, queries)
        assert lookup(text, heads, names * 2) == name_cases.want_found(names, queries)         # duplicates do not count as distinct
    d_text, n = on_device(text)
    with ff.NameSet([b'one']) as s:
        assert ff.fastq_name_lookup(d_text, n, heads[:0], s).tolist() == []                      # no records: nothing is launched


def test_a_nearly_full_table_and_more_records_than_a_grid_round(libmpn):
    many = [b'name_%d' % i for i in range(63)]
    queries = many + [b'absent_%d' % i for i in range(64)] + many[::-1]
    text, heads = text_of(queries)
    assert lookup(text, heads, many, slots=64) == name_cases.want_found(many, queries)       # chains that run long and wrap the end
    one = [b'one', b'two'] * 35_000
    text, heads = text_of(one, seq_len=lambda k: 1)
    got = lookup(text, heads, [b'one'], slots=16)
    assert len(got) == 70_000 and got == [0, -1] * 35_000


def test_bad_arguments_return_minus_2_and_launch_nothing(libmpn, all_ids):
    from megapath_nano_amd import _ffi, fastq_filter as ff
    for slots, names in ((48, [b'a']), (16, [b'%d' % i for i in range(16)]), (1, [b'a']), (-16, [b'a'])):
        with pytest.raises(_ffi.MpnError, match='rc=-2'):
            ff.NameSet(names, slots)
    text, heads = text_of(all_ids[:4])
    d_text, n = on_device(text)
    with ff.NameSet(all_ids) as s:
        for field, value in (('off', n + 1), ('off', n - 1), ('off', -1), ('id_len', -1), ('off', 1 << 40)):
            bad = heads.copy()
            bad[field][2] = value
            with pytest.raises(_ffi.MpnError, match='rc=-2'):
                ff.fastq_name_lookup(d_text, n, bad, s)
            assert ff.last_lookup_device_ms() == 0
        assert ff.fastq_name_lookup(d_text, n, heads, s).tolist() == [0, 1, 2, 3]
        assert ff.last_lookup_device_ms() > 0
    with pytest.raises(_ffi.MpnError, match='rc=-2'):                # a closed set is a NULL set
        ff.fastq_name_lookup(d_text, n, heads, s)
