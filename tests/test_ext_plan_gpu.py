"""GPU tests (-m gpu) of the extension planning stage (csrc/plan_kernels.h: plan_kernel, plan_hit, pk_filter_bad_seeds, AnchorView --
mm_fix_bad_ends, mm_filter_bad_seeds, the limits of the end extensions and the cut of a hit into windows) through its stage entry
point mpn_ext_plan_batch, which runs the launch function the mapper's alignment rounds run.  Every per-hit field, every field of
every window and every anchor word the kernel leaves behind is compared with the sequential restatement of plan_ref.py, exact
integers; test_plan_ref.py pins that restatement to the oracle's own align1 on the same cases and asserts that the families of
plan_cases.py reach what they are here for: the 1024 anchors the kernel stages in LDS, the 8192 its bit mask covers, the word
boundaries of that mask, trimmed hits whose mask positions and anchor indices differ, flags written to two copies.  Each batch runs
with the mapper's grid and with a single block, which then takes every hit in turn on the same LDS arrays."""
import numpy as np
import pytest

from plan_cases import FAMILIES, families
from plan_ref import HIT_KEYS, WIN_KEYS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib(libmpn):
    return libmpn


@pytest.fixture(scope='module')
def fams():
    return families()


@pytest.fixture(scope='module')
def refs(fams):
    """plan_ref of every read of every batch, computed once and left unchanged"""
    return {name: [b.ref() for b in batches] for name, batches in fams.items()}


def run(b, arrays, grid_cap):
    from megapath_nano_amd import mapper
    opt = mapper.default_opt(**b.opt)
    return mapper.ext_plan_batch(opt, b.k, arrays['tlens'], arrays['q_len'], arrays['anchor_off'], arrays['anchors'], arrays['hit_off'],
                                 arrays['h_as'], arrays['h_cnt'], arrays['h_mlen'], arrays['h_split_inv'], grid_cap=grid_cap)


def check(family, b, want, grid_cap):
    from megapath_nano_amd import mapper
    assert mapper.PLAN_HIT_KEYS == HIT_KEYS and mapper.PLAN_WIN_KEYS == ('read',) + WIN_KEYS
    arrays = b.arrays()
    hits, wins, left = run(b, arrays, grid_cap)
    where = (family, b.name, 'grid_cap %d' % grid_cap)
    assert len(hits) == sum(len(r.hits) for r in b.reads), where
    assert len(wins) == sum(h['n_jobs'] for whits, _, _ in want for h in whits), where + ('windows', len(wins))
    hp = wp = 0
    for ri, (r, (whits, _, _)) in enumerate(zip(b.reads, want)):
        for hi, (spec, wh) in enumerate(zip(r.hits, whits)):
            at = where + ('read %d %s' % (ri, r.name), 'hit %d (as %d, cnt %d)' % (hi, spec[0], spec[1]))
            for j, key in enumerate(HIT_KEYS):
                assert int(hits[hp, j]) == wh[key], at + (key, int(hits[hp, j]), wh[key])
            for wi, ww in enumerate(wh['windows']):
                assert int(wins[wp, 0]) == ri, at + ('window %d' % wi, 'read', int(wins[wp, 0]), ri)
                for j, key in enumerate(WIN_KEYS):
                    assert int(wins[wp, 1 + j]) == ww[key], at + ('window %d' % wi, key, int(wins[wp, 1 + j]), ww[key])
                wp += 1
            hp += 1
    assert wp == len(wins)
    wleft = np.array([p for _, a, _ in want for p in a], dtype=np.uint64).reshape(-1, 2)
    if not np.array_equal(left, wleft):
        bad = int(np.nonzero((left != wleft).any(axis=1))[0][0])
        ri = int(np.searchsorted(arrays['anchor_off'], bad, side='right')) - 1
        ai = bad - int(arrays['anchor_off'][ri])
        hi = [k for k, (as_, cnt, _, _) in enumerate(b.reads[ri].hits) if as_ <= ai < as_ + cnt]
        assert False, where + ('read %d %s' % (ri, b.reads[ri].name), 'hit %s' % (hi[0] if hi else 'none'), 'anchor %d' % ai,
                               [hex(int(v)) for v in left[bad]], [hex(int(v)) for v in wleft[bad]])


@pytest.mark.parametrize('grid_cap', [0, 1])
@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_family_equals_ref(lib, fams, refs, family, grid_cap):
    for b, want in zip(fams[family], refs[family]):
        check(family, b, want, grid_cap)


def test_blocks_share_hits_evenly_or_not_at_all(lib, fams, refs):
    """a grid of two and of three blocks over the batch whose hits differ most in size: the stride of the hit loop"""
    b, want = fams['batch'][0], refs['batch'][0]
    for grid_cap in (2, 3):
        check('batch', b, want, grid_cap)


def test_bad_input_is_refused_before_any_launch(lib, fams):
    from megapath_nano_amd import _ffi
    b = fams['neighbours'][0]

    def broken(change):
        arrays = {k: v.copy() for k, v in b.arrays().items()}
        change(arrays)
        with pytest.raises(_ffi.MpnError, match='mpn_ext_plan_batch: read 0: '):       # (the validation's words, not a device error's)
            run(b, arrays, 0)

    first = int(b.arrays()['h_as'][0])        # the first hit of the first read (its read's list starts the anchor array)

    def zero_cnt(a):
        a['h_cnt'][0] = 0

    def beyond(a):
        a['h_cnt'][0] = int(a['anchor_off'][1]) - first + 1

    def overlap(a):
        a['hit_off'][1:] += 1
        for key in ('h_as', 'h_cnt', 'h_mlen', 'h_split_inv'):
            a[key] = np.concatenate([a[key][:1], a[key]])

    def two_targets(a):
        a['anchors'][first + 1, 0] ^= np.uint64(1 << 32)

    def bad_rid(a):
        a['anchors'][:, 0] |= np.uint64(7 << 32)

    def beyond_target(a):
        a['tlens'][:] = 100

    def beyond_read(a):
        a['q_len'][0] = 10

    def x_not_increasing(a):
        a['anchors'][first + 1, 0] = a['anchors'][first, 0]

    def y_not_increasing(a):
        a['anchors'][first + 2, 1] = a['anchors'][first + 1, 1]

    def no_span(a):
        a['anchors'][first, 1] &= np.uint64(0xffffff00ffffffff)

    def unknown_flag(a):
        a['anchors'][first, 1] |= np.uint64(1 << 43)

    def no_length(a):
        a['q_len'][0] = 0

    for change in (zero_cnt, beyond, overlap, two_targets, bad_rid, beyond_target, beyond_read, x_not_increasing, y_not_increasing, no_span,
                   unknown_flag, no_length):
        broken(change)
