"""CPU: tests/filter_ref.py (the header rule and the record text the read filter on the device adds) is pinned to the host filter
and, through it, to the reference binary: on every case of both nanofastq goldens, the data flow of the device path restated --
fastq_scan_ref.scan, heads_ref, the oracle's sums, fastq_filter.decide, emit_ref, and parse_fastx + assemble from the first record the
scan does not take -- reproduces the binary's stdout and stderr byte for byte.  The same test holds the factoring of assemble()."""
import json
import math
import os

import numpy as np
import pytest

import fastq_scan_ref as scan_ref
import filter_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = {name: json.load(open(os.path.join(ROOT, 'tests', 'golden', name + '.json'))) for name in ('nanofastq_golden', 'nanofastq_edges_golden')}
CASES = [(g, k) for g, gold in GOLDENS.items() for k in range(len(gold['cases']))]


def kw_of(args):
    keys = {'-q': 'min_quality', '-l': 'min_length', '-h': 'head_crop', '-t': 'tail_crop', '-r': 'read_id_prefix'}
    return {keys[a]: (v if a == '-r' else int(v)) for a, v in zip(args[::2], args[1::2])}


def restated(text, kw):
    """the device path's data flow with the restatements in place of the kernels -> (stdout, stderr, records the scan took)"""
    from megapath_nano_amd import fastq_filter as ff
    from oracle import fastq_oracle as fo
    h, t = kw.get('head_crop', 0), kw.get('tail_crop', 0)
    min_len = max(kw.get('min_length', 0), 1)
    prefix = kw.get('read_id_prefix')
    rows, consumed, status = scan_ref.scan(text, True)
    heads = filter_ref.heads_ref(text, rows)
    keep, picks, lines = [], [], []
    for k, (w, hd) in enumerate(zip(rows, heads)):
        l, off = int(w['len']), int(hd['off'])
        total, cropped = fo.qsums(text[int(w['qual_off']):int(w['qual_off']) + l], h, t, min_len)
        rid = ff.read_id(text[off:off + int(hd['id_len'])], k + 1, prefix)
        passed, line = ff.decide(rid, l, True, total, cropped, kw.get('min_quality', 0), min_len, h, t)
        lines.append(line)
        if passed:
            keep.append(k)
            picks.append((h, l - h - t, int(hd['comment_len']) > 0, k + 1 if prefix is not None else 0))
    out = filter_ref.emit_ref(text, rows[keep], heads[keep], filter_ref.picks_of(picks), (prefix or '').encode())
    info = b''.join(lines)
    if status == scan_ref.UNSUPPORTED:
        recs = ff._parse_text(text[consumed:])
        total, cropped = np.zeros(len(recs)), np.zeros(len(recs))
        for k, r in enumerate(recs):
            if r[3] is not None:
                total[k], cropped[k] = fo.qsums(r[3], h, t, min_len)
        o, i, _ = ff.assemble(recs, total, cropped, first=len(rows), **kw)
        out, info = out + o, info + i
    return out, info, len(rows)


@pytest.mark.parametrize('gold,k', CASES, ids=[f'{g}-{k}' for g, k in CASES])
def test_restated_device_flow_reproduces_the_reference_binary(gold, k):
    c = GOLDENS[gold]['cases'][k]
    text = GOLDENS[gold]['inputs'][c['input']].encode('latin-1')
    out, info, _ = restated(text, kw_of(c['args']))
    assert out.decode('latin-1') == c['stdout']
    assert info.decode('latin-1') == c['stderr']


def test_the_goldens_reach_both_paths_and_the_edges():
    taken = {}
    for gold in GOLDENS.values():
        for name, text in gold['inputs'].items():
            text = text.encode('latin-1')
            rows, consumed, status = scan_ref.scan(text, True)
            taken[name] = (len(rows), consumed < len(text))
    # whole inputs on the device, inputs that hand over in the middle, and one the host takes from its second record
    assert taken['ont_like'] == (16, False) and taken['headers'][1] is False and taken['crlf'][1] is False
    assert taken['mixed_small'][1] and taken['multiline'][1] and taken['perfect_and_awful'] == (3, True)
    edges = GOLDENS['nanofastq_edges_golden']
    assert len(edges['cases']) == 15
    assert any(c['input'] == 'serials' and '@p_9\n' not in c['stdout'] and '@p_10 ' in c['stdout'] for c in edges['cases'])
    assert not any(ch in text for text in edges['inputs'].values() for ch in '\v\f')      # not the host mirror's rule


def test_heads_ref_is_parse_fastx_on_every_plain_record():
    from megapath_nano_amd import fastq_filter as ff
    texts = [g['inputs'][n].encode('latin-1') for g in GOLDENS.values() for n in g['inputs']]
    texts += [t for _, t, final in scan_ref.plain_cases(scan_ref.header_tile()) if final and b'\x0b' not in t and b'\x0c' not in t]
    texts.append(b'@a\x0bb\x0cc d\nAC\n+\nII\n')            # VT and FF stay inside the id
    seen = 0
    for text in texts:
        rows, consumed, _ = scan_ref.scan(text, True)
        heads = filter_ref.heads_ref(text, rows)
        recs = ff._parse_text(text[:consumed])
        if any(int(w['len']) == 0 for w in rows):
            continue                                       # (an empty read: parse_fastx reads the '+' line as bases)
        assert len(recs) == len(rows)
        for w, h, (name, comment, seq, qual) in zip(rows, heads, recs):
            off, n, c = int(h['off']), int(h['id_len']), int(h['comment_len'])
            assert text[off:off + n] == name and text[off - 1:off] == b'@'
            assert (text[off + n + 1:off + n + 1 + c] if c > 0 else None) == comment
            assert text[int(w['seq_off']):int(w['seq_off']) + int(w['len'])] == seq
            seen += 1
    assert seen > 3000


def test_decide_is_the_code_assemble_runs():
    """one decision and line for both paths, with math.log10 (libm, as the C program) and the -0.00 of a perfect score"""
    from megapath_nano_amd import fastq_filter as ff
    passed, line = ff.decide(b'r', 4, True, np.float64(4.0), np.float64(2.0), 0, 1, 1, 1)
    assert (passed, line) == (1, b'r\t4\t-0.00\t2\t-0.00\t1\n') and math.copysign(1, -10 * math.log10(1.0)) == -1
    out, info, kept = ff.assemble([(b'r', None, b'ACGT', b'!!!!')], [4.0], [2.0], head_crop=1, tail_crop=1)
    assert (out, info, kept) == (b'@r\nCG\n+\n!!\n', line, [('r', b'CG')])
