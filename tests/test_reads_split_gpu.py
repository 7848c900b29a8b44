"""GPU tests (-m gpu) of mpn_reads_split_plan and mpn_reads_split_gather (include/mpn_reads.h; csrc/interval_kernels.hip and
csrc/read_split_kernels.hip): on every case of tests/split_cases.py the device plan and the gathered bytes equal the numpy
statement exactly -- every byte of [0, out_bytes), zero padding included, bases and qualities, from host and from device sources --
and the 64 guard bytes behind out_bytes come back untouched.  Bad arguments are refused before anything is launched."""
import ctypes as ct

import numpy as np
import pytest

import split_cases

pytestmark = pytest.mark.gpu

CASES = split_cases.make_cases()
GUARD = 64


def _guarded(torch, out_bytes):
    return torch.full((out_bytes + GUARD,), 0xEE, dtype=torch.uint8, device='cuda')


@pytest.mark.parametrize('i', range(len(CASES)), ids=[c['name'] for c in CASES])
def test_device_plan_equals_the_host_form(libmpn, i):
    from megapath_nano_amd import mapper
    c, want = CASES[i], split_cases.expected(i)
    got = mapper.device_split_plan(c['lens'], c['mem_read'], c['mem_group'], c['n_groups'])
    split_cases.assert_same(dict(got, seqs=None, quals=None), dict(want, seqs=None, quals=None), c['name'])


@pytest.mark.parametrize('source', ['host', 'device'])
@pytest.mark.parametrize('i', range(len(CASES)), ids=[c['name'] for c in CASES])
def test_device_gather_equals_the_host_form_and_keeps_its_bounds(libmpn, i, source):
    import torch
    from megapath_nano_amd import mapper
    c, want = CASES[i], split_cases.expected(i)
    plan = {k: want[k] for k in mapper.PLAN_KEYS}
    with_q = c['qbuf'] is not None
    d_out, d_qout = _guarded(torch, want['out_bytes']), (_guarded(torch, want['out_bytes']) if with_q else None)
    dev_src = None
    if source == 'device':   # the sources as they are, without a byte behind them that the host buffer does not have
        dev_src = (torch.from_numpy(c['buf']).cuda(), torch.from_numpy(c['qbuf']).cuda() if with_q else None)
    h, hq = mapper.device_split_gather(plan, c['buf'], c['off'], c['lens'], d_out[:want['out_bytes']], c['qbuf'],
                                       d_qout[:want['out_bytes']] if with_q else None, dev_src)
    torch.cuda.synchronize()
    for name, dev, host, exp in (('seqs', d_out, h, want['seqs']), ('quals', d_qout, hq, want['quals'])):
        if exp is None:
            assert dev is None and host is None
            continue
        back = dev.cpu().numpy()
        assert (back[want['out_bytes']:] == 0xEE).all(), (c['name'], name, 'bytes behind out_bytes were written')
        bad = np.flatnonzero(back[:want['out_bytes']] != exp)
        assert len(bad) == 0, (c['name'], name, source, 'first difference at byte', int(bad[0]), int(back[bad[0]]), int(exp[bad[0]]), len(bad), 'differ')
        assert np.array_equal(host, exp), (c['name'], name, 'host copy')


def test_device_split_reads_returns_what_the_host_form_returns(libmpn):
    from megapath_nano_amd import mapper
    for i in (0, 3):
        c, want = CASES[i], split_cases.expected(i)
        got = mapper.device_split_reads(c['buf'], c['off'], c['lens'], c['mem_read'], c['mem_group'], c['n_groups'], c['qbuf'])
        split_cases.assert_same(got, want, c['name'])
        assert np.array_equal(got['d_seqs'].cpu().numpy(), want['seqs']) and np.array_equal(got['d_quals'].cpu().numpy(), want['quals'])


def test_split_reads_of_a_resident_batch_gives_resident_group_views(libmpn):
    import torch
    from megapath_nano_amd import mapper
    rng = np.random.default_rng(5)
    seqs = [bytes(rng.choice(np.frombuffer(b'ACGT', dtype=np.uint8), size=int(l))) for l in (40, 0, 1000, 17, 3000, 5)]
    names = [f'r{i}' for i in range(len(seqs))]
    packed = mapper.PackedReads(names, seqs, device='cuda')
    sp = mapper.split_reads(packed, [4, 0, 2, 5, 2, 1], [0, 0, 1, 1, 0, 1], 3)                 # device=None: where the batch is
    for g, reads in enumerate(([0, 2, 4], [1, 2, 5], [])):
        p = sp.group(g)
        assert p.names == [names[r] for r in reads] and p.dev is not None and p.dev[0].data_ptr() % 16 == 0
        off, lens, buf = p.dev[1].cpu().numpy(), p.dev[2].cpu().numpy(), p.dev[0].cpu().numpy()
        assert np.array_equal(off, p.off) and np.array_equal(lens, p.lens)
        assert [buf[o:o + l].tobytes() for o, l in zip(off, lens)] == [seqs[r] for r in reads] == [p.seq(k).tobytes() for k in range(p.n)]
        assert p.dev[0].data_ptr() == sp.res['d_seqs'].data_ptr() + int(sp.res['group_byte'][g])           # a view, not a copy
    torch.cuda.synchronize()


def test_bad_arguments_are_refused_before_anything_is_launched(libmpn):
    import torch
    from megapath_nano_amd import _ffi, mapper
    lib = mapper._bind()
    i32, i64 = (lambda v: np.ascontiguousarray(v, dtype=np.int32)), (lambda v: np.ascontiguousarray(v, dtype=np.int64))
    lens = i32([5, 7, 0])

    def plan(lens=lens, n=3, mem_read=(0, 1), mem_group=(0, 1), n_groups=2, cap=None, null=None):
        mr, mg = i32(mem_read), i32(mem_group)
        m = len(mr)
        out_read, out_off = np.full(8, -7, dtype=np.int32), np.full(8, -7, dtype=np.int64)
        first, gbyte = np.full(n_groups + 1, -7, dtype=np.int64), np.full(n_groups + 1, -7, dtype=np.int64)
        n_out, out_bytes = ct.c_int64(-7), ct.c_int64(-7)
        args = dict(len=lens.ctypes.data, mem_read=mr.ctypes.data, mem_group=mg.ctypes.data, n_out=ct.addressof(n_out), out_read=out_read.ctypes.data,
                    group_first=first.ctypes.data, out_off=out_off.ctypes.data, group_byte=gbyte.ctypes.data, out_bytes=ct.addressof(out_bytes))
        if null:
            args[null] = None
        rc = lib.mpn_reads_split_plan(n, args['len'], m, args['mem_read'], args['mem_group'], n_groups, m if cap is None else cap, args['n_out'],
                                      args['out_read'], args['group_first'], args['out_off'], args['group_byte'], args['out_bytes'])
        return rc, (out_read, out_off, n_out.value)

    assert plan()[0] == 0
    for what, kw in (('negative length', dict(lens=i32([5, -1, 0]))), ('read >= n', dict(mem_read=(0, 3))), ('read < 0', dict(mem_read=(-1, 1))),
                     ('group >= n_groups', dict(mem_group=(0, 2))), ('group < 0', dict(mem_group=(0, -1))), ('negative n', dict(n=-1)),
                     ('negative n_groups', dict(n_groups=-1, mem_read=(), mem_group=())), ('null len', dict(null='len')),
                     ('null mem_read', dict(null='mem_read')), ('null out_off', dict(null='out_off')), ('null n_out', dict(null='n_out')),
                     ('null group_byte', dict(null='group_byte'))):
        rc, (out_read, out_off, _) = plan(**kw)
        assert rc == -1 and 'mpn_reads_split_plan' in _ffi.last_error(), what
        assert (out_read == -7).all() and (out_off == -7).all(), what
    rc, _ = plan(mem_read=(0, 1, 2), mem_group=(0, 0, 1), cap=2)                       # three output reads, room for two
    assert rc == -1 and 'room for 2' in _ffi.last_error()

    c, want = CASES[3], split_cases.expected(3)
    off, lens, buf = c['off'], c['lens'], c['buf']
    src_bytes = int((off + lens).max())
    out_read, out_off = want['out_read'], want['out_off']

    def gather(n=len(lens), seqs=buf.ctypes.data, src_bytes=src_bytes, off=off, lens=lens, n_out=want['n_out'], out_read=out_read, out_off=out_off,
               out_bytes=want['out_bytes'], cap=None, shift=0, null_out=False):
        d_out = _guarded(torch, want['out_bytes'])
        rc = lib.mpn_reads_split_gather(n, seqs, None, src_bytes, off.ctypes.data, lens.ctypes.data, 0, n_out, out_read.ctypes.data, out_off.ctypes.data,
                                        out_bytes, None if null_out else d_out.data_ptr() + shift, None, want['out_bytes'] if cap is None else cap, None, None)
        torch.cuda.synchronize()
        return rc, d_out.cpu().numpy()

    rc, back = gather()
    assert rc == 0 and np.array_equal(back[:want['out_bytes']], want['seqs'])
    bad_off = off.copy()
    bad_off[2] = -1
    overlap = out_off.copy()
    overlap[1] -= 1
    beyond = out_off.copy()
    beyond[-1] = want['out_bytes'] - 1
    for what, kw in (('negative offset', dict(off=bad_off)), ('negative length', dict(lens=i32(np.where(np.arange(len(lens)) == 1, -1, lens)))),
                     ('read beyond the source', dict(src_bytes=src_bytes - 1)), ('out_read outside', dict(out_read=i32(np.where(np.arange(len(out_read)) == 0, len(lens), out_read)))),
                     ('overlapping output reads', dict(out_off=overlap)), ('output read beyond out_bytes', dict(out_off=beyond)),
                     ('out_bytes not a multiple of 16', dict(out_bytes=want['out_bytes'] - 8)), ('capacity too small', dict(cap=want['out_bytes'] - 16)),
                     ('unaligned output', dict(shift=4)), ('null output', dict(null_out=True)), ('null source', dict(seqs=None)),
                     ('negative n_out', dict(n_out=-1))):
        rc, back = gather(**kw)
        assert rc == -1 and 'mpn_reads_split_gather' in _ffi.last_error(), what
        assert (back == 0xEE).all(), (what, 'the output was written')
