"""CPU tests (no GPU) of index parts sharded over ranks: the rank layout, the part assignment, the owner
sub-ranges of a batch, the byte exchange over gloo with world 2, and the refusals of the hits block that need no mapping."""
import json
import os
import socket
import subprocess
import sys
import textwrap

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_index_shard_layout():
    from megapath_nano_amd.dist import index_shard_layout
    assert [index_shard_layout(r, 8, 2) for r in range(8)] == [(g, s) for g in range(4) for s in range(2)]
    assert [index_shard_layout(r, 4, 4) for r in range(4)] == [(0, 0), (0, 1), (0, 2), (0, 3)]
    assert [index_shard_layout(r, 3, 1) for r in range(3)] == [(0, 0), (1, 0), (2, 0)]
    for bad in ((0, 6, 4), (0, 4, 0), (4, 4, 2), (-1, 4, 2)):
        with pytest.raises(ValueError):
            index_shard_layout(*bad)


def _check_assignment(bases, n_shards):
    from megapath_nano_amd.dist import assign_parts
    blocks = assign_parts(bases, n_shards)
    assert len(blocks) == n_shards and blocks[0][0] == 0 and blocks[-1][1] == len(bases)
    assert all(a < b for a, b in blocks), blocks                             # every shard holds a part
    assert all(blocks[s][1] == blocks[s + 1][0] for s in range(n_shards - 1))  # contiguous, in target order
    sums = [int(np.sum(bases[a:b])) for a, b in blocks]
    assert max(sums) <= sum(bases) / n_shards + max(bases), (sums, bases)     # balanced by bases
    assert assign_parts(list(bases), n_shards) == blocks                      # a pure function of the part list
    return blocks


def test_part_assignment_contiguous_balanced_deterministic():
    from megapath_nano_amd.dist import assign_parts
    rng = np.random.default_rng(5)
    for n_parts in (1, 2, 3, 4, 7, 30, 200):
        bases = rng.integers(1, 4_000_000_000, size=n_parts)
        for s in range(1, min(n_parts, 8) + 1):
            _check_assignment(bases, s)
        assert assign_parts(bases, 1) == [(0, n_parts)]                       # S = 1: one block
    assert _check_assignment(np.array([5, 5, 5, 5]), 2) == [(0, 2), (2, 4)]
    assert _check_assignment(np.array([1, 1, 1, 100]), 2) == [(0, 3), (3, 4)]  # a large last part still leaves a block for each
    assert _check_assignment(np.array([100, 1, 1, 1]), 3) == [(0, 1), (1, 2), (2, 4)]
    with pytest.raises(ValueError):
        assign_parts([10, 10], 3)


def test_owner_ranges_cover_every_read_once():
    from megapath_nano_amd.dist import owner_bounds, index_shard_layout
    rng = np.random.default_rng(9)
    for n_reads in (0, 1, 3, 10, 1000):
        lens = rng.integers(200, 30000, size=n_reads)
        for world, S in ((1, 1), (2, 2), (4, 2), (8, 4), (6, 3), (8, 1), (16, 8)):
            groups, owned = owner_bounds(lens, world // S, S)
            assert len(groups) == world // S and len(owned) == world
            assert owned[0][0] == 0 and owned[-1][1] == n_reads
            assert all(owned[r][1] == owned[r + 1][0] for r in range(world - 1))     # contiguous in rank order
            assert all(lo <= hi for lo, hi in owned)                                  # (empty ranges allowed)
            cover = np.zeros(n_reads, dtype=np.int64)
            for lo, hi in owned:
                cover[lo:hi] += 1
            assert (cover == 1).all()
            for r in range(world):                                                    # rank (g, s) owns a piece of group g
                g, s = index_shard_layout(r, world, S)
                assert groups[g][0] <= owned[r][0] <= owned[r][1] <= groups[g][1]
    _, owned = owner_bounds([5000, 7000], 4, 2)                                      # more ranks than reads
    assert sum(hi > lo for lo, hi in owned) <= 2 and sum(hi - lo for lo, hi in owned) == 2


def test_hits_block_refusals_without_mapping(libmpn):
    """Header-level refusals of mpn_hits_import on blocks of empty accumulators (the GPU test covers blocks with hits)."""
    from megapath_nano_amd import mapper
    from megapath_nano_amd._ffi import MpnError
    p = mapper.PackedReads(['a', 'b', 'c'], [b'ACGT' * 10, b'AC' * 30, b'GGG'])
    src = mapper.Hits(p, want_text=False)
    blk = src.export(0, 3)
    assert len(blk) == src.export(0, 3).nbytes and blk[:4].tobytes() == b'MPHB'
    acc = mapper.Hits(p, want_text=False)
    with pytest.raises(MpnError):
        acc.import_block(blk, 1, ['x'], [10])                  # target list other than the exporter's
    with pytest.raises(MpnError):
        mapper.Hits(p.sub(0, 2), want_text=False).import_block(blk, 0, [], [])   # read count
    with pytest.raises(MpnError):
        mapper.Hits(p, want_text=True).import_block(blk, 0, [], [])              # want_text
    for cut in list(range(0, 65)) + [len(blk) - 1]:
        if cut < len(blk):
            with pytest.raises(MpnError):
                acc.import_block(blk[:cut], 0, [], [])
    bad = blk.copy()
    bad[0] ^= 0xff
    with pytest.raises(MpnError):
        acc.import_block(bad, 0, [], [])
    bad = blk.copy()
    bad[-1] ^= 1
    with pytest.raises(MpnError):
        acc.import_block(bad, 0, [], [])
    acc.import_block(blk, 0, [], [])
    with pytest.raises(MpnError):
        src.export(2, 4)
    src.close()
    acc.close()


def test_packed_sub_range():
    from megapath_nano_amd import mapper
    seqs = [b'ACGTA', b'', b'GGCCTTAA', b'T' * 13]
    quals = [b'IIIII', b'', b'########', b'5' * 13]
    p = mapper.PackedReads(['r0', 'r1', 'r2', 'r3'], seqs, quals=quals)
    for lo, hi in ((0, 4), (1, 3), (2, 4), (3, 3), (0, 0), (4, 4)):
        s = p.sub(lo, hi)
        assert s.n == hi - lo and s.names == p.names[lo:hi] and s.bases == sum(len(x) for x in seqs[lo:hi])
        assert [bytes(s.seq(i)) for i in range(s.n)] == seqs[lo:hi]
        assert [bytes(s.qbuf[s.off[i]:s.off[i] + s.lens[i]]) for i in range(s.n)] == quals[lo:hi]
        assert len(s.buf) >= s.bases + 4 and (s.n == 0 or s.off[0] == 0)
        assert [x.decode() for x in s.cnames] == s.names and s.dev is None


GLOO_EXCHANGE = textwrap.dedent('''
    import os, sys, json
    import numpy as np
    sys.path.insert(0, %r)
    from megapath_nano_amd import dist as mdist
    rank, world, _ = mdist.init_from_env(backend='gloo')
    sizes = [[0, 5, 70000], [3, 0, 1]][rank]                 # uneven and empty blocks; block j goes to rank j
    out = {}
    for step, sz in enumerate(sizes):
        blocks = [np.full(sz + 7 * j, (rank * 16 + j * 4 + step) %% 256, dtype=np.uint8) if sz or j else np.zeros(0, np.uint8)
                  for j in range(world)]
        got = mdist.exchange_bytes(blocks, None)
        out[step] = [[int(len(g)), sorted(set(g.tolist()))] for g in got]
    empty = mdist.exchange_bytes([np.zeros(0, np.uint8)] * world, None)
    out['empty'] = [len(g) for g in empty]
    groups = mdist.shard_groups(world, 2)
    out['groups'] = len(groups)
    with open(os.path.join(os.environ['MPN_TEST_OUT'], f'x{rank}.json'), 'w') as f:
        json.dump(out, f)
''')


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def test_exchange_bytes_gloo_world2(tmp_path):
    script = tmp_path / 'worker.py'
    script.write_text(GLOO_EXCHANGE % ROOT)
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE='2', LOCAL_RANK=str(r), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                   MPN_TEST_OUT=str(tmp_path))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    errs = []
    try:
        for p in procs:
            _, err = p.communicate(timeout=240)
            errs.append(err)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), [e[-2000:] for e in errs]
    res = [json.load(open(tmp_path / f'x{r}.json')) for r in range(2)]
    sizes = [[0, 5, 70000], [3, 0, 1]]
    for me in range(2):
        for step in range(3):
            for src in range(2):
                sz = sizes[src][step]
                n = sz + 7 * me if (sz or me) else 0
                want = [n, [(src * 16 + me * 4 + step) % 256] if n else []]
                assert res[me][str(step)][src] == want, (me, step, src, res[me][str(step)][src], want)
        assert res[me]['empty'] == [0, 0] and res[me]['groups'] == 1
