"""GPU tests (-m gpu) of mpn_gzip_inflate (csrc/inflate_kernels.hip): many gzip streams inflated on the GPU, one wave per stream.
zlib is the judge (tests/test_inflate_cases.py pins the cases to it on the CPU, and runs them through the host build of the same
decoder).  Every case of inflate_cases.py goes through the entry point in one call, alone and in a shuffled call."""
import numpy as np
import pytest

import inflate_cases as ic

pytestmark = pytest.mark.gpu
FILL = 0xA5


def run(ingest, streams, caps):
    """-> list of (status, members, length, the slot's bytes -- all of the slot, so that what the call left alone shows)"""
    n = len(streams)
    in_off = np.zeros(n + 1, dtype=np.int64)
    in_off[1:] = np.cumsum([len(s) for s in streams])
    data = np.frombuffer(b''.join(streams) + b'\0', dtype=np.uint8)
    caps = np.array(caps, dtype=np.int64)
    slot_off = np.zeros(n + 1, dtype=np.int64)
    slot_off[1:] = np.cumsum((caps + 16 + 15) & ~15)          # 16 bytes of guard at least behind every slot
    out = np.full(int(slot_off[-1]) + 16, FILL, dtype=np.uint8)
    length, members, status = ingest.inflate_host(n, data, in_off, slot_off[:n], caps, out)
    return [(int(status[i]), int(members[i]), int(length[i]), out[slot_off[i]:slot_off[i + 1]].tobytes()) for i in range(n)]


def full_cap(c):
    return len(c['data']) if c['data'] is not None else 1 << 16


def check(c, got, cap):
    status, members, length, slot = got
    assert status == c['status'], (c['name'], status)
    if c['status'] == ic.OK:
        assert (members, length) == (c['members'], len(c['data'])), c['name']
        assert slot[:length] == c['data'], c['name']
        assert slot[length:] == bytes([FILL]) * (len(slot) - length), c['name'] + ': bytes behind the stream were written'
    else:
        assert slot[cap:] == bytes([FILL]) * (len(slot) - cap), c['name'] + ': bytes behind the slot were written'


@pytest.fixture(scope='module')
def ingest(libmpn):
    from megapath_nano_amd import ingest
    return ingest


@pytest.fixture(scope='module')
def cases():
    return ic.make_cases()


def test_all_cases_in_one_call(ingest, cases):
    got = run(ingest, [c['gz'] for c in cases], [full_cap(c) for c in cases])
    for c, g in zip(cases, got):
        check(c, g, full_cap(c))


def test_every_case_alone(ingest, cases):
    for c in cases:
        check(c, run(ingest, [c['gz']], [full_cap(c)])[0], full_cap(c))


def test_shuffled_order(ingest, cases):
    order = np.random.default_rng(9).permutation(len(cases))
    mixed = [cases[i] for i in order]
    got = run(ingest, [c['gz'] for c in mixed], [full_cap(c) for c in mixed])
    for c, g in zip(mixed, got):
        check(c, g, full_cap(c))


def test_small_slot_overflows_with_the_exact_length(ingest, cases):
    """Every second valid case gets a slot of half its size (one gets none at all): OVERFLOW, the exact length and member count, the
    first bytes in the slot, nothing behind it -- and the neighbours, which have full slots, as if nothing had happened."""
    valid = [c for c in cases if c['status'] == ic.OK]
    caps = [len(c['data']) // 2 if k % 2 and len(c['data']) > 1 else len(c['data']) for k, c in enumerate(valid)]
    first_small = next(k for k, c in enumerate(valid) if caps[k] < len(c['data']))
    caps[first_small] = 0
    got = run(ingest, [c['gz'] for c in valid], caps)
    n_small = 0
    for c, cap, (status, members, length, slot) in zip(valid, caps, got):
        if cap == len(c['data']):
            check(c, (status, members, length, slot), cap)
            continue
        n_small += 1
        assert (status, members, length) == (ic.OVERFLOW, c['members'], len(c['data'])), c['name']
        assert slot[:cap] == c['data'][:cap] and slot[cap:] == bytes([FILL]) * (len(slot) - cap), c['name']
    assert n_small > 20


def test_wrapper_retries_an_overflow_once(ingest, cases):
    """inflate_files sizes a slot from the LAST member's ISIZE: the multi-member files overflow it and come back right from the one
    retry; the malformed ones keep their status."""
    inf = ingest.inflate_files([c['gz'] for c in cases])
    by_name = {c['name']: k for k, c in enumerate(cases)}
    assert {by_name[x] for x in ('two_members', 'five_members', 'bgzf_with_eof', 'mid_byte_then_member')} <= set(inf.retried)
    for k, c in enumerate(cases):
        assert int(inf.status[k]) == c['status'], c['name']
        if c['status'] == ic.OK:
            assert int(inf.members[k]) == c['members'] and inf.bytes(k) == c['data'], c['name']
    assert inf.on_host == [] and inf.launches == 2          # the retried streams went in ONE further launch


def test_oversized_stream_is_inflated_by_zlib(ingest, cases):
    picked = [c for c in cases if c['name'] in ('fasta_300000_l6', 'flag_all', 'two_members')]
    inf = ingest.inflate_files([c['gz'] for c in picked], limit=1000)
    assert inf.on_host == [k for k, c in enumerate(picked) if len(c['gz']) > 1000] and len(inf.on_host) == 2
    for k, c in enumerate(picked):
        assert int(inf.status[k]) == ic.OK and inf.bytes(k) == c['data'], c['name']


def test_device_time_is_reported(ingest, cases):
    run(ingest, [cases[0]['gz']], [full_cap(cases[0])])
    inflate_ms, _ = ingest.last_device_ms()
    assert 0 < inflate_ms < 10_000
