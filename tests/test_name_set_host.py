"""CPU tests of what nanosplit on the device adds below the GPU: the name set of csrc/name_set_core.h, built and probed on the host by
scripts/name_set_host_check.cpp (plain g++; the functions are the ones the lookup kernel calls) against a Python dict, and the numpy
plan of fastx.split_emit_plan / fastx.emit_rounds against a loop over dicts."""
import os
import struct
import subprocess

import numpy as np
import pytest

from megapath_nano_amd import fastx

import fastq_scan_ref as scan_ref
import filter_ref
import name_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp('name_set') / 'name_set_host_check'
    subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-o', str(path), os.path.join(ROOT, 'scripts', 'name_set_host_check.cpp')], check=True)
    return path


def run_host_check(exe, tmp_path, cases):
    """cases: [(slots, names, queries)] -> [(rc, slots, distinct, first_of, found, slots read)]"""
    src, dst = tmp_path / 'cases.bin', tmp_path / 'results.bin'
    with open(src, 'wb') as f:
        f.write(struct.pack('<I', len(cases)))
        for slots, names, queries in cases:
            f.write(struct.pack('<qQ', slots, len(names)) + b''.join(struct.pack('<Q', len(x)) + x for x in names))
            f.write(struct.pack('<Q', len(queries)) + b''.join(struct.pack('<Q', len(x)) + x for x in queries))
    subprocess.run([str(exe), str(src), str(dst)], check=True, timeout=300)
    blob, out, p = dst.read_bytes(), [], 0
    for slots, names, queries in cases:
        rc, = struct.unpack_from('<i', blob, p)
        p += 4
        if rc:
            out.append((rc, None, None, None, None, None))
            continue
        got_slots, distinct = struct.unpack_from('<qq', blob, p)
        p += 16
        first_of = list(struct.unpack_from(f'<{len(names)}i', blob, p))
        p += 4 * len(names)
        pairs = struct.unpack_from(f'<{2 * len(queries)}i', blob, p)
        p += 8 * len(queries)
        out.append((rc, got_slots, distinct, first_of, list(pairs[0::2]), list(pairs[1::2])))
    assert p == len(blob)
    return out


def test_host_build_of_the_name_set_agrees_with_a_dict(exe, tmp_path):
    ids = name_cases.ids()
    absent = [b'absent', b'', ids[3] + b'\0', ids[9][:-1], ids[9] + b'y', b'\0' * 16, ids[10][:39]]
    cases = []
    for names in (ids, ids[::-1], ids + ids[::-1] + ids[:5], [], [b'one'], [b''], [b'', b'', b'x'],
                  [b'n%d' % i for i in range(8)], [b'n%d' % i for i in range(9)]):
        cases.append((0, names, ids + absent))
    many = [b'name_%d' % i for i in range(63)]
    cases.append((64, many, many + absent))                      # 63 of 64 slots: chains that run long and wrap the end
    cases.append((16, [b'one'], [b'one'] * 3 + absent))
    for (slots, names, queries), (rc, got_slots, distinct, first_of, found, seen) in zip(cases, run_host_check(exe, tmp_path, cases)):
        assert rc == 0
        assert distinct == len(set(names)) and got_slots == (slots or name_cases.default_slots(distinct))
        assert first_of == name_cases.want_found(names, names)
        assert found == name_cases.want_found(names, queries)
        assert all(1 <= k <= got_slots for k in seen)
    assert [c[1] for c in run_host_check(exe, tmp_path, [(0, [b'n%d' % i for i in range(k)], []) for k in (8, 9)])] == [16, 32]
    # 63 names in 64 slots: one empty slot, so the absent names walk to it -- some chain is long, and some walk passes the table's end
    seen = run_host_check(exe, tmp_path, [(64, many, [b'absent_%d' % i for i in range(64)])])[0][5]
    assert max(seen) > 16
    # slots that are no power of two, or not larger than the number of distinct names
    for slots, names in ((48, [b'a']), (16, [b'%d' % i for i in range(16)]), (-16, [b'a']), (1, [b'a']), (2, [b'a', b'b'])):
        assert run_host_check(exe, tmp_path, [(slots, names, [])])[0][0] == -2, slots
    assert run_host_check(exe, tmp_path, [(2, [b'a', b'a'], [b'a'])])[0][:5] == (0, 2, 1, [0, 0], [0])     # distinct names count, not entries


# ---- the plan --------------------------------------------------------------------------------------------------------------------
def plan_case(records, wanted, n_outputs):
    """records: [(header bytes behind the '@', bases)]; wanted: {id: sorted outputs} -> (text, rows, heads, found, name_ptr, name_out)"""
    text = b''.join(scan_ref.rec(h, s, scan_ref._quals(len(s), k)) for k, (h, s) in enumerate(records))
    rows, consumed, status = scan_ref.scan(text, True)
    assert consumed == len(text) and status == scan_ref.OK and len(rows) == len(records)
    heads = filter_ref.heads_ref(text, rows)
    names = list(wanted)
    ids = [text[int(h['off']):int(h['off']) + int(h['id_len'])] for h in heads]
    found = np.array(name_cases.want_found(names, ids), dtype=np.int32)
    name_ptr = np.cumsum([0] + [len(wanted[k]) for k in names])
    name_out = np.array([g for k in names for g in wanted[k]], dtype=np.int64)
    return text, rows, heads, found, name_ptr, name_out


def files_by_dicts(records, wanted, n_outputs):
    """what the host path of fastx.nanosplit writes per output, restated"""
    out = [b''] * n_outputs
    for k, (h, s) in enumerate(records):
        cut = min((h.find(c) for c in (b' ', b'\t') if c in h), default=len(h))
        name, comment = h[:cut], h[cut + 1:]
        for g in wanted.get(name, ()):
            out[g] += b'@' + name + (b' ' + comment if comment else b'') + b'\n' + s + b'\n+\n' + scan_ref._quals(len(s), k) + b'\n'
    return out


def plan_cases():
    every = list(range(1000))
    recs = [(b'none', b'ACGT'), (b'one c', b'ACGTA'), (b'every', b'AC'), (b'twice', b'A' * 40), (b'twice x', b'C' * 33), (b'empty', b''),
            (b'blank ', b'ACG'), (b'tab\tc d', b'GG'), (b'', b'T'), (b'big', b'ACGT' * 300)]
    wanted = {b'one': [2, 1001], b'every': every, b'twice': [0, 2], b'empty': [0, 999], b'blank': [2], b'tab': [5], b'': [5], b'big': [2, 7],
              b'absent': [1000]}
    yield 'mixed', recs, wanted, 1003
    yield 'zero_records', [], wanted, 1003
    yield 'nothing_listed', recs, {}, 3
    yield 'none_found', recs[:1], wanted, 1003
    yield 'empty_reads', [(b'e%d' % i, b'') for i in range(5)], {b'e0': [0], b'e3': [0, 1], b'e4': [1]}, 2


@pytest.mark.parametrize('case', list(plan_cases()), ids=[c[0] for c in plan_cases()])
def test_plan_equals_the_loop_over_dicts(case):
    _, records, wanted, n_outputs = case
    text, rows, heads, found, name_ptr, name_out = plan_case(records, wanted, n_outputs)
    want = files_by_dicts(records, wanted, n_outputs)
    plan = fastx.split_emit_plan(found, name_ptr, name_out, n_outputs, heads, rows)
    n = len(plan.rec)
    assert n == sum(len(wanted.get(h[:min((h.find(c) for c in (b' ', b'\t') if c in h), default=len(h))], ())) for h, _ in records)
    key = plan.out.astype(np.int64) << 32 | plan.rec
    assert (np.diff(key) > 0).all()                                               # sorted by (output, record), a pair once
    assert plan.pair_first[0] == 0 and plan.pair_first[-1] == n and len(plan.pair_first) == n_outputs + 1
    sizes = filter_ref.sizes_ref(text, rows[plan.rec], heads[plan.rec], plan.picks)
    assert plan.out_off[0] == 0 and (np.diff(plan.out_off) == sizes).all()
    assert (plan.picks['start'] == 0).all() and (plan.picks['serial'] == 0).all() and (plan.picks['m'] == rows['len'][plan.rec]).all()
    whole = filter_ref.emit_ref(text, rows[plan.rec], heads[plan.rec], plan.picks)
    for g in range(n_outputs):
        a, b = int(plan.out_off[plan.pair_first[g]]), int(plan.out_off[plan.pair_first[g + 1]])
        assert whole[a:b] == want[g], g
        assert (plan.out[plan.pair_first[g]:plan.pair_first[g + 1]] == g).all()
    # the same files from rounds of any size: a round is consecutive pairs, at least one, at most the limit unless it is one pair
    for limit in (1, 64, 700, 1 << 20):
        rounds = fastx.emit_rounds(plan.out_off, limit)
        assert [a for a, _ in rounds] + [n] == [0] + [b for _, b in rounds] if n else rounds == []       # they tile the pairs
        got = [b''] * n_outputs
        for a, b in rounds:
            assert b > a and (plan.out_off[b] - plan.out_off[a] <= limit or b == a + 1)
            assert b == n or plan.out_off[b + 1] - plan.out_off[a] > limit            # greedy: the next pair would not fit
            part = filter_ref.emit_ref(text, rows[plan.rec[a:b]], heads[plan.rec[a:b]], plan.picks[a:b])
            for j in range(a, b):
                got[int(plan.out[j])] += part[int(plan.out_off[j] - plan.out_off[a]):int(plan.out_off[j + 1] - plan.out_off[a])]
        assert got == want, limit


def test_plan_cases_are_the_ones_promised():
    name, records, wanted, n_outputs = next(plan_cases())
    text, rows, heads, found, name_ptr, name_out = plan_case(records, wanted, n_outputs)
    plan = fastx.split_emit_plan(found, name_ptr, name_out, n_outputs, heads, rows)
    per_record = np.bincount(plan.rec, minlength=len(records))
    assert per_record[0] == 0 and per_record[6] == 1 and per_record[2] == 1000               # in no output, in one, in each of 1000
    counts = np.diff(plan.pair_first)
    assert counts[999] == 2 and counts[1000] == 0 and counts[1001] == 1 and counts[1002] == 0   # an empty output between full ones, and at the end
    assert counts[1] == 1 and counts[2] > 1 and counts[0] > 1
    assert found[3] == found[4] >= 0 and per_record[3] == per_record[4] == 2                 # the same name in two records
    assert heads['comment_len'].tolist()[:9] == [-1, 1, -1, -1, 1, -1, 0, 3, -1]             # absent, present, and empty (`@blank ` + LF)
    assert plan.picks['with_comment'][plan.rec == 6].tolist() == [0] and plan.picks['with_comment'][plan.rec == 7].tolist() == [1]
    assert heads['id_len'][8] == 0 and per_record[8] == 1                                    # an empty id that is listed
    sizes = np.diff(plan.out_off)
    assert sizes.max() > 700 and len(fastx.emit_rounds(plan.out_off, 700)) > 3               # a record larger than a round; several rounds
    assert len(fastx.emit_rounds(plan.out_off, 1)) == len(plan.rec)
