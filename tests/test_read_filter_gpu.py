"""GPU tests (-m gpu) of the read filter on the device (MPN_READ_INGEST=device): mpn_fastq_heads, mpn_fastq_qsum_rows and
mpn_fastq_emit on their own against oracle.fastq_oracle.qsums and tests/filter_ref.py, on rows of the restated scan
(tests/fastq_scan_ref.py); then fastq_filter.filter_stream / filter_fastx, bin/mpn-nanofastq and fastx.subseq against the host path
(the knob unset) and the reference binary's goldens."""
import ctypes as ct
import gzip
import io
import json
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import fastq_scan_ref as scan_ref
import filter_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = {name: json.load(open(os.path.join(ROOT, 'tests', 'golden', name + '.json'))) for name in ('nanofastq_golden', 'nanofastq_edges_golden')}
SUM_LENS = (1, 15, 16, 17, 4095, 4096, 4097, 9000)
# (head crop, tail crop, min_len); the last two leave exactly min_len of the reads of 17 and of 4096 bases (and less of the next shorter)
CROPS = ((0, 0, 1), (50, 30, 1), (8000, 8000, 1), (0, 1, 1), (10, 6, 1), (3000, 1000, 96))


def kw_of(args):
    keys = {'-q': 'min_quality', '-l': 'min_length', '-h': 'head_crop', '-t': 'tail_crop', '-r': 'read_id_prefix'}
    return {keys[a]: (v if a == '-r' else int(v)) for a, v in zip(args[::2], args[1::2])}


def on_device(text):
    """-> (uint8 device tensor of the text and 16 bytes behind it, the text's length)"""
    import torch
    return torch.from_numpy(np.frombuffer(bytes(text) + b'\0' * 16, dtype=np.uint8).copy()).cuda(), len(text)


def rows_of(text):
    rows, consumed, status = scan_ref.scan(text, True)
    assert consumed == len(text) and status == scan_ref.OK
    return rows


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv('MPN_INGEST_BATCH_BYTES', '65536')
    monkeypatch.delenv('MPN_READ_INGEST', raising=False)


# ---- sums ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sum_text():
    """reads of every length of SUM_LENS behind headers of 1 .. 17 bytes, and the oracle's sums per crop"""
    from oracle import fastq_oracle as fo
    rng = np.random.default_rng(18)
    parts = []
    for h in range(1, 18):
        for n in SUM_LENS:
            parts.append(scan_ref.rec(b'h' * h, scan_ref._bases(n, h), bytes(rng.integers(33, 33 + 61, size=n, dtype=np.uint8))))
    text = b''.join(parts)
    rows = rows_of(text)
    assert len(rows) == 17 * len(SUM_LENS) and {int(o) % 16 for o in rows['qual_off']} == set(range(16))
    want = {}
    for h, t, m in CROPS:
        want[h, t, m] = [fo.qsums(text[int(w['qual_off']):int(w['qual_off']) + int(w['len'])], h, t, m) for w in rows]
    return text, rows, want


@pytest.mark.parametrize('order', ['as_scanned', 'reversed', 'by_length'])
def test_sums_are_the_oracles_doubles(libmpn, sum_text, order):
    from megapath_nano_amd import fastq_filter as ff
    text, rows, want = sum_text
    d_text, n = on_device(text)
    pick = {'as_scanned': np.arange(len(rows)), 'reversed': np.arange(len(rows))[::-1], 'by_length': np.argsort(rows['len'], kind='stable')}[order]
    for (h, t, m), sums in want.items():
        for by_length in (False, True):
            total, cropped, status = ff.qsum_rows(d_text, n, rows[pick], h, t, m, by_length=by_length)
            assert not status.any()
            for k, r in enumerate(pick.tolist()):
                assert (total[k], cropped[k]) == sums[r], (h, t, m, by_length, r)          # exact doubles, not a tolerance
    # the crops that leave exactly min_len are taken, one base less is not
    lens = rows['len'].tolist()
    for (h, t, m), l in (((10, 6, 1), 17), ((3000, 1000, 96), 4096)):
        k = lens.index(l)
        assert want[h, t, m][k][1] != want[h, t, m][k][0] and l - h - t == m
        k = lens.index(l - 1)
        assert want[h, t, m][k][1] == want[h, t, m][k][0]


def test_a_bad_quality_character_flags_its_read_only(libmpn):
    from megapath_nano_amd import fastq_filter as ff
    from oracle import fastq_oracle as fo
    rng = np.random.default_rng(3)
    quals = [bytearray(rng.integers(33, 33 + 61, size=100, dtype=np.uint8).tobytes()) for _ in range(7)]
    for k, pos, byte in ((1, 3, 0x1f), (3, 50, 0xc8), (5, 97, 0x20 - 1)):         # the first, an inner and the last 16 bytes of a read
        quals[k][pos] = byte
    text = b''.join(scan_ref.rec(b'b%d' % k, scan_ref._bases(100, k), bytes(q)) for k, q in enumerate(quals))
    rows = rows_of(text)
    d_text, n = on_device(text)
    for by_length in (False, True):
        total, cropped, status = ff.qsum_rows(d_text, n, rows, 5, 5, 1, by_length=by_length)
        assert status.tolist() == [0, 1, 0, 1, 0, 1, 0]
        for k in range(7):
            assert (total[k], cropped[k]) == ((0.0, 0.0) if k % 2 else fo.qsums(bytes(quals[k]), 5, 5, 1))


# ---- heads ---------------------------------------------------------------------------------------------------------------------
def head_texts(tile):
    edges = GOLDENS['nanofastq_edges_golden']['inputs']
    out = {name: edges[name].encode('latin-1') for name in ('headers', 'crlf', 'qual_at', 'no_last_lf')}
    out.update({'ref_' + c[0]: c[1] for c in scan_ref.plain_cases(tile) if c[0] in ('long_header', 'names', 'qual_starts', 'crlf')})
    first = scan_ref.rec(b'x' * (tile - 20) + b' spans the\ttile', b'ACGT')             # the first record: line start 0; its header spans the tile edge
    out['first_spans_tile'] = first + scan_ref.rec(b'n', b'AC', b'@I') + scan_ref.rec(b'after_at c', b'ACG')
    out['header_5000'] = scan_ref.GOOD[0] + scan_ref.rec(b'i' * 1200 + b'\t' + b'c d ' * 950, b'ACGTA') + scan_ref.GOOD[1]
    return out


def test_heads_follow_the_host_filters_rule(libmpn):
    from megapath_nano_amd import fastq_filter as ff, ingest
    texts = head_texts(ingest.fastq_tile())
    assert len(texts['header_5000'].split(b'\n')[4]) == 1 + 5001
    seen = set()
    for name, text in texts.items():
        rows = rows_of(text)
        want = filter_ref.heads_ref(text, rows)
        d_text, n = on_device(text)
        for pick in (np.arange(len(rows)), np.arange(len(rows))[::-1], np.arange(len(rows))[1::2]):      # not only consecutive rows
            heads, ids = ff.fastq_heads(d_text, n, rows[pick])
            assert heads.tolist() == want[pick].tolist(), name
            assert ids == [text[int(h['off']):int(h['off']) + int(h['id_len'])] for h in want[pick]], name
            assert ff.fastq_heads(d_text, n, rows[pick], with_ids=False)[0].tolist() == want[pick].tolist()
        seen |= {(int(h['id_len']) == 0, int(h['comment_len']) < 0, int(h['comment_len']) == 0) for h in want}
        # and they are parse_fastx's names and comments
        recs = ff._parse_text(text)
        assert len(recs) == len(rows)
        for h, rec in zip(want, recs):
            off, k, c = int(h['off']), int(h['id_len']), int(h['comment_len'])
            assert (text[off:off + k], text[off + k + 1:off + k + 1 + c] if c > 0 else None) == rec[:2], name
    assert {(True, False, False), (True, True, False), (False, False, True), (False, True, False)} <= seen      # '@ a x', '@', '@a ', '@plain'
    text = texts['headers']
    assert text.startswith(b'@a \n') and b'\n@a\tx y\n' in text and b'\n@a  x\n' in text and b'\n@ a x\n' in text and b'\n@\n' in text


def test_heads_reject_rows_outside_the_text(libmpn):
    from megapath_nano_amd import _ffi, fastq_filter as ff
    text = scan_ref.GOOD[0] + scan_ref.GOOD[1]
    rows = rows_of(text)
    d_text, n = on_device(text)
    for field, value in (('seq_off', 1), ('seq_off', n + 1), ('len', -1), ('qual_off', n), ('qual_off', 1 << 40)):
        bad = rows.copy()
        bad[field][1] = value
        with pytest.raises(_ffi.MpnError, match='rc=-2'):
            ff.fastq_heads(d_text, n, bad)
        if (field, value) != ('seq_off', 1):               # (the sums do not need a header line in front of the bases)
            with pytest.raises(_ffi.MpnError, match='rc=-2'):
                ff.qsum_rows(d_text, n, bad, 0, 0, 1)


# ---- emit ----------------------------------------------------------------------------------------------------------------------
def emit_both(text, rows, heads, items, prefix=b''):
    """mpn_fastq_emit through its wrapper and emit_ref on the same records -> (device bytes with the padding, reference bytes)"""
    from megapath_nano_amd import fastq_filter as ff
    d_text, n = on_device(text)
    picks = filter_ref.picks_of(items)
    d_out, out_off = ff.fastq_emit(d_text, n, rows, heads, picks, prefix)
    want = filter_ref.emit_ref(text, rows, heads, picks, prefix)
    assert np.array_equal(np.diff(out_off), filter_ref.sizes_ref(text, rows, heads, picks, prefix)) and int(out_off[-1]) == len(want)
    return d_out.cpu().numpy().tobytes(), want


def assert_emitted(got, want):
    padded = (len(want) + 15) & ~15
    assert len(got) >= padded and got[:len(want)] == want and got[len(want):padded] == b'\0' * (padded - len(want))


def test_emit_at_every_alignment_and_across_short_records(libmpn):
    text = dict((c[0], c[1]) for c in scan_ref.plain_cases(4096))['short_3000'] + scan_ref.rec(b'tail comment', scan_ref._bases(333), scan_ref._quals(333))
    rows = rows_of(text)
    heads = filter_ref.heads_ref(text, rows)
    items = [(0, int(l), 1, 0) for l in rows['len']]
    got, want = emit_both(text, rows, heads, items)
    assert_emitted(got, want)
    starts = np.cumsum([0] + filter_ref.sizes_ref(text, rows, heads, filter_ref.picks_of(items)).tolist())
    assert {int(s) % 16 for s in starts} == set(range(16))
    # one-base reads, 9 bytes a record, in a run of 200; and a subset in reversed order
    text = b''.join(scan_ref.rec(b'abcdefghij'[i % 10:i % 10 + 1], b'ACGT'[i % 4:i % 4 + 1], scan_ref._quals(1, i)) for i in range(200))
    rows = rows_of(text)
    heads = filter_ref.heads_ref(text, rows)
    got, want = emit_both(text, rows, heads, [(0, 1, 0, 0)] * 200)
    assert len(want) == 9 * 200
    assert_emitted(got, want)
    pick = np.arange(200)[::-3]
    got, want = emit_both(text, rows[pick], heads[pick], [(0, 1, 1, 0)] * len(pick))
    assert_emitted(got, want)


def test_emit_crops_drops_and_nothing(libmpn):
    from megapath_nano_amd import fastq_filter as ff
    text = b''.join(scan_ref.rec(b'd%d c' % i, scan_ref._bases(20 + i % 50, i), scan_ref._quals(20 + i % 50, i)) for i in range(1001))
    rows = rows_of(text)
    heads = filter_ref.heads_ref(text, rows)
    got, want = emit_both(text, rows[1000:], heads[1000:], [(3, 5, 1, 0)])            # one kept behind 1000 dropped ones
    assert want == b'@d1000 c\n' + text[int(rows[1000]['seq_off']) + 3:][:5] + b'\n+\n' + text[int(rows[1000]['qual_off']) + 3:][:5] + b'\n'
    assert_emitted(got, want)
    items = [(int(l) - 1 - k % 2 * (int(l) - 1), 1, k % 2, 0) for k, l in enumerate(rows['len'])]       # crops that leave the last / the first base
    got, want = emit_both(text, rows, heads, items)
    assert_emitted(got, want)
    d_text, n = on_device(text)
    d_out, out_off = ff.fastq_emit(d_text, n, rows[:0], heads[:0], filter_ref.picks_of([]))         # none kept: an empty output, return 0
    assert out_off.tolist() == [0]


def test_emit_serials_and_the_comment_flag(libmpn):
    text = b''.join(scan_ref.rec(h, b'ACGTAC', b'IIII@+') for h in (b'a ', b'b some comment', b'c', b'a ', b'e\tx', b' f'))
    rows = rows_of(text)
    heads = filter_ref.heads_ref(text, rows)
    serials = (9, 10, 99, 100, 999_999, 1_000_000)
    for prefix in (b'', b'p' * 39 + b'_'):
        got, want = emit_both(text, rows, heads, [(1, 4, k % 2, s) for k, s in enumerate(serials)], prefix)
        assert_emitted(got, want)
        assert want.startswith(b'@' + prefix + b'9\nCGTA\n+\nIII@\n@' + prefix + b'10 some comment\n') and b'@' + prefix + b'1000000 f\n' in want
    # '@a ': nanofastq leaves the blank out (no comment), subseq keeps it (a separator was found)
    for flag, line in ((0, b'@a\n'), (1, b'@a \n')):
        got, want = emit_both(text, rows[:1], heads[:1], [(0, 6, flag, 0)])
        assert want.startswith(line)
        assert_emitted(got, want)


def test_emit_takes_a_second_round_of_the_grid(libmpn):
    n_reads, l = 1100, 4000                                          # > 2048 blocks x 4 waves x 1024 bytes of output
    parts = [scan_ref.rec(b'g%04d c' % i, scan_ref._bases(l, i % 7), scan_ref._quals(l, i % 5)) for i in range(n_reads)]
    text = b''.join(parts)
    size = len(parts[0])
    rows = np.zeros(n_reads, dtype=scan_ref.ROW)
    rows['seq_off'] = np.arange(n_reads) * size + 9
    rows['qual_off'] = rows['seq_off'] + l + 3
    rows['name_off'], rows['len'], rows['name_len'] = np.arange(n_reads) * size + 1, l, 5
    assert text[int(rows[-1]['seq_off']) - 9:][:9] == b'@g1099 c\n' and text[int(rows[-1]['qual_off']) - 3:][:3] == b'\n+\n'
    heads = np.zeros(n_reads, dtype=filter_ref.HEAD)
    heads['off'], heads['id_len'], heads['comment_len'] = rows['name_off'], 5, 1
    assert heads[:3].tolist() == filter_ref.heads_ref(text, rows[:3]).tolist()
    got, want = emit_both(text, rows, heads, [(1, l - 2, 1, 0)] * n_reads)
    assert len(want) > 2048 * 4 * 1024
    assert_emitted(got, want)


def test_emit_checks_out_off_and_out_cap_before_it_writes(libmpn):
    import torch
    from megapath_nano_amd import fastq_filter as ff
    lib = ff._dev_lib()
    text = scan_ref.GOOD[0] + scan_ref.GOOD[1] + scan_ref.GOOD[2]
    rows = rows_of(text)
    heads = filter_ref.heads_ref(text, rows)
    picks = filter_ref.picks_of([(0, int(l), 0, 0) for l in rows['len']])
    good = np.concatenate([[0], np.cumsum(filter_ref.sizes_ref(text, rows, heads, picks))]).astype(np.int64)
    d_text, n = on_device(text)
    need = (int(good[-1]) + 15) & ~15

    def call(out_off, cap):
        d_out = torch.full((need + 64,), 0xaa, dtype=torch.uint8, device='cuda')
        rc = lib.mpn_fastq_emit(d_text.data_ptr(), n, len(rows), rows.ctypes.data, heads.ctypes.data, picks.ctypes.data, b'', 0,
                                out_off.ctypes.data, d_out.data_ptr(), cap)
        return rc, d_out.cpu().numpy()

    rc, out = call(good, need)
    assert rc == 0 and out[:good[-1]].tobytes() == filter_ref.emit_ref(text, rows, heads, picks) and (out[need:] == 0xaa).all()
    for k, d in ((1, 1), (1, -1), (3, 1), (0, 1)):
        wrong = good.copy()
        wrong[k] += d
        rc, out = call(wrong, need + 64)
        assert rc == -2 and (out == 0xaa).all(), (k, d)
    rc, out = call(good, need - 16)
    assert rc == -2 and (out == 0xaa).all()


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def host_and_device(data, monkeypatch, **kw):
    from megapath_nano_amd import fastq_filter as ff
    monkeypatch.delenv('MPN_READ_INGEST', raising=False)
    want = ff.filter_fastx(data, **kw)
    monkeypatch.setenv('MPN_READ_INGEST', 'device')
    got = ff.filter_fastx(data, **kw)
    monkeypatch.delenv('MPN_READ_INGEST')
    return got, want


@pytest.mark.parametrize('gold', sorted(GOLDENS))
def test_device_path_is_the_host_path_on_the_goldens(libmpn, monkeypatch, gold):
    n_fallback = 0
    for c in GOLDENS[gold]['cases']:
        text = GOLDENS[gold]['inputs'][c['input']].encode('latin-1')
        got, want = host_and_device(text, monkeypatch, **kw_of(c['args']))
        assert got == want, (c['input'], c['args'])                                # stdout, stderr and the kept reads
        assert (want[0].decode('latin-1'), want[1].decode('latin-1')) == (c['stdout'], c['stderr'])
        rows, consumed, _ = scan_ref.scan(text, True)
        n_fallback += 0 < len(rows) and consumed < len(text) and '-r' in c['args']
    assert n_fallback > 0 or gold != 'nanofastq_golden'          # -r serials run on through the hand-over in the middle of a stream


def bgzf_block(payload):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    data = c.compress(payload) + c.flush()
    return (b'\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0' + struct.pack('<H', len(data) + 25) + data +
            struct.pack('<II', zlib.crc32(payload) & 0xffffffff, len(payload)))


def test_texts_cut_inside_records_and_the_compressed_forms(libmpn, monkeypatch):
    gold = GOLDENS['nanofastq_golden']
    text = gold['inputs']['ont_like'].encode('latin-1')
    monkeypatch.setenv('MPN_INGEST_BATCH_BYTES', '5000')             # records straddle the carry: most reads are longer than a text
    for c in gold['cases']:
        if c['input'] == 'ont_like':
            got, want = host_and_device(text, monkeypatch, **kw_of(c['args']))
            assert got == want and want[0].decode('latin-1') == c['stdout'], c['args']
    three = text * 3
    assert len(three) > 2 * (1 << 16)
    block = 1 << 16
    forms = {'gzip': gzip.compress(three, 6),
             'bgzf': b''.join(bgzf_block(three[a:a + block - 256]) for a in range(0, len(three), block - 256)) + bgzf_block(b'')}
    kw = dict(min_quality=7, min_length=500, head_crop=50, tail_crop=30, read_id_prefix='s_')
    for size in ('5000', '100000'):
        monkeypatch.setenv('MPN_INGEST_BATCH_BYTES', size)
        plain = host_and_device(three, monkeypatch, **kw)
        assert plain[0] == plain[1] and plain[1][0].count(b'\n') >= 4
        for form, data in forms.items():
            got, want = host_and_device(data, monkeypatch, **kw)
            assert got == want == plain[1], (form, size)
    # the same bytes could come from a path that hands everything to the host: the stage clock says where the records went
    from megapath_nano_amd import fastq_filter as ff
    for data, on_device_records, on_host in ((forms['bgzf'], 48, False), (gold['inputs']['perfect_and_awful'].encode('latin-1'), 3, True),
                                            (gold['inputs']['mixed_small'].encode('latin-1'), 0, True)):
        t = {}
        reads, kept = ff.filter_stream(io.BytesIO(data), io.BytesIO(), io.BytesIO(), timings=t)
        assert (t.get('records', 0), 'host' in t) == (on_device_records, on_host) and reads >= max(on_device_records, 4) and kept == reads
        assert not on_device_records or min(t['heads_device_ms'], t['sums_device_ms'], t['emit_device_ms']) > 0


def test_errors_are_the_host_paths_and_earlier_texts_stay_written(libmpn, monkeypatch):
    from megapath_nano_amd import fastq_filter as ff
    good = b''.join(scan_ref.rec(b'g%d' % i, scan_ref._bases(900, i), scan_ref._quals(900, i)) for i in range(8))
    monkeypatch.setenv('MPN_INGEST_BATCH_BYTES', '4000')
    for bad in (scan_ref.rec(b'empty', b'', b''), scan_ref.rec(b'badq', b'ACGT', b'II\x1fI')):
        for data in (bad + good, good + bad + good):
            with pytest.raises(ValueError) as host:
                ff.filter_fastx(data)
            monkeypatch.setenv('MPN_READ_INGEST', 'device')
            with pytest.raises(ValueError) as dev:
                ff.filter_fastx(data)
            out, info = io.BytesIO(), io.BytesIO()
            with pytest.raises(ValueError):
                ff.filter_stream(io.BytesIO(data), out, info)
            monkeypatch.delenv('MPN_READ_INGEST')
            assert str(dev.value) == str(host.value)                  # 'empty read NAME: ..' / 'read N holds ..'
            # the texts in front of the one with the bad read were filtered and written
            if data.startswith(good):
                assert out.getvalue().startswith(good[:len(scan_ref.rec(b'g0', scan_ref._bases(900, 0), scan_ref._quals(900, 0)))])
                assert out.getvalue() == good[:len(out.getvalue())] and info.getvalue().count(b'\n') == out.getvalue().count(b'\n') // 4
            else:
                assert out.getvalue() == b''
    with pytest.raises(ValueError):
        ff.filter_stream(io.BytesIO(good), io.BytesIO(), io.BytesIO(), head_crop=-1)
    assert ff.filter_stream(io.BytesIO(good), io.BytesIO(), io.BytesIO(), min_length=901) == (8, 0)
    assert ff.filter_stream(io.BytesIO(b''), io.BytesIO(), io.BytesIO()) == (0, 0)


def test_batches_hold_the_kept_reads_cropped(libmpn, monkeypatch):
    from megapath_nano_amd import fastq_filter as ff, ingest
    gold = GOLDENS['nanofastq_golden']
    kw = dict(min_quality=7, min_length=100, head_crop=50, tail_crop=30)
    for name, prefix in (('ont_like', None), ('ont_like', 'x_'), ('multiline', None), ('perfect_and_awful', 'y'), ('mixed_small', None)):
        text = gold['inputs'][name].encode('latin-1')
        opts = dict(kw, read_id_prefix=prefix) if name != 'perfect_and_awful' else dict(read_id_prefix=prefix)
        out, info, kept = ff.filter_fastx(text, **opts)                            # the host path
        fq = [r for r in ff.parse_fastx(out)]
        monkeypatch.setenv('MPN_INGEST_BATCH_BYTES', '5000')
        batcher = ingest.ReadBatcher(6000, 'cuda')
        o, i = io.BytesIO(), io.BytesIO()
        got = list(ff.filter_stream(io.BytesIO(text), o, i, batches=batcher, **opts)) + list(batcher.flush())
        assert (o.getvalue(), i.getvalue()) == (out, info)
        reads = [(b.names[k], b.buf[b.off[k]:b.off[k] + b.lens[k]].tobytes(), None if b.qbuf is None else b.qbuf[b.off[k]:b.off[k] + b.lens[k]].tobytes())
                 for b in got for k in range(b.n)]
        assert [(n, s) for n, s, _ in reads] == kept, name
        for (n, s, q), (rn, _, rs, rq) in zip(reads, fq):
            assert s == rs and (q == rq or (rq is None and q in (None, b'!' * len(s)))), name
        assert len(reads) == len(fq) and (len(got) > 1 or name != 'ont_like')


def test_executable_streams_stdin_and_rejects_an_unknown_knob(libmpn):
    exe = [sys.executable, os.path.join(ROOT, 'bin', 'mpn-nanofastq')]
    gold = GOLDENS['nanofastq_golden']
    c = next(c for c in gold['cases'] if c['input'] == 'ont_like' and '-r' in c['args'])
    data = gold['inputs']['ont_like'].encode('latin-1')
    p = subprocess.run(exe + c['args'], input=data, capture_output=True, timeout=300, env=dict(os.environ, MPN_READ_INGEST='device', MPN_INGEST_BATCH_BYTES='20000'))
    assert p.returncode == 0, p.stderr[-500:]
    assert p.stdout.decode('latin-1') == c['stdout'] and p.stderr.decode('latin-1') == c['stderr']
    p = subprocess.run(exe + c['args'], input=data, capture_output=True, timeout=300, env=dict(os.environ, MPN_READ_INGEST='bogus'))
    assert p.returncode != 0 and p.stdout == b'' and b'MPN_READ_INGEST=bogus' in p.stderr


def test_subseq_on_the_device_writes_the_hosts_bytes(libmpn, monkeypatch, tmp_path):
    from megapath_nano_amd import fastx
    recs = [scan_ref.rec(b'r%d' % i + (b' comment %d' % i if i % 3 else b''), scan_ref._bases(300 + i, i), scan_ref._quals(300 + i, i)) for i in range(30)]
    recs[4] = scan_ref.rec(b'blank ', b'ACGTAC', b'@IIII+')                      # a trailing blank: subseq keeps it
    recs[7] = scan_ref.rec(b'tab\t', b'ACGTA')
    text = b''.join(recs[:20]) + b'>fasta in the middle\nACGTACGT\nACGT\n' + b''.join(recs[20:])
    names = ['r1', 'r2', 'blank', 'tab', 'r19', 'fasta', 'r20', 'r29', 'absent']
    for form, data in (('plain', text), ('gz', gzip.compress(text)), ('bgzf', b''.join(bgzf_block(text[a:a + 3000]) for a in range(0, len(text), 3000)))):
        path = tmp_path / f'in.{form}'
        path.write_bytes(data)
        for size in ('2000', '65536'):
            monkeypatch.setenv('MPN_INGEST_BATCH_BYTES', size)
            monkeypatch.delenv('MPN_READ_INGEST', raising=False)
            want = io.BytesIO()
            n_want = fastx.subseq(str(path), names, want)
            monkeypatch.setenv('MPN_READ_INGEST', 'device')
            got = io.BytesIO()
            assert fastx.subseq(str(path), names, got) == n_want == 8
            assert got.getvalue() == want.getvalue()
            assert b'@blank \n' in want.getvalue() and b'@tab \n' in want.getvalue() and b'>fasta in the middle\n' in want.getvalue()
    # a FASTA file takes the host path from its first byte
    (tmp_path / 'f.fa').write_bytes(b'>f x\nACGT\n>g\nAC\n')
    got = io.BytesIO()
    assert fastx.subseq(str(tmp_path / 'f.fa'), ['g'], got) == 1 and got.getvalue() == b'>g\nAC\n'
