"""GPU tests (-m gpu) of Clair's network (megapath_nano_amd/clair_net.py, csrc/clair_net_kernels.hip) against the restatement
(tests/clair_net_ref.py), with seeded weights at the initialiser's scale.

The accuracy rule: per tap and for the probabilities, the device's largest absolute deviation from the restatement in float64 is at
most 4 x that of the restatement in float32 on the CPU on the same inputs.  Two input families: counts (tensors of the tensor
goldens and random integers in [0, 100], which saturate the gates) and integers in [0, 3] (which keep them sensitive).  Where a
constructed weight set leaves a tap so simple that the float32 run hits the float64 values almost exactly, the yardstick has the
floor of half a float32 ulp of the tap's largest value (2^-24 x max |value|): no float32 evaluation can promise less.

Rows are independent and every sum is ordered, so batch and chunk edges are checked bitwise against the same tensor run alone."""
import io
import os
import random
import subprocess
import sys
import ctypes as ct

import numpy as np
import pytest

import clair_net_ref as ref
import tensor_cases as tc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'bin', 'mpn-call-var')
CTG = 'ctgT'
NAMES = ref.TAPS + ('probs',)


@pytest.fixture(scope='module')
def cn(libmpn):
    from megapath_nano_amd import clair_net
    return clair_net


@pytest.fixture(scope='module')
def weights():
    return ref.seeded_weights(7)


@pytest.fixture(scope='module')
def net(cn, weights):
    os.environ.pop('MPN_CLAIR_CHUNK', None)
    n = cn.ClairNet(weights)
    yield n
    n.close()


@pytest.fixture(scope='module')
def families(cn):
    """{family: (n, 33, 8, 4) int32}, 2 x MPN_CLAIR_TILE + 3 tensors each"""
    n = 2 * cn.tile() + 3
    return {'counts': ref.counts_inputs(n, 31), 'small': ref.small_inputs(n, 32)}


@pytest.fixture(scope='module')
def expected(weights, families):
    """{family: (probs64, taps64, yardsticks)}: computed once, shared, never changed"""
    return {k: ref.deviations(weights, v) for k, v in families.items()}


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda()


def run(net, x, taps=True):
    probs, t = net.predict(dev(x), taps=True)
    got = {k: v.cpu().numpy() for k, v in t.items()}
    got['probs'] = probs.cpu().numpy()
    return got


def check(got, p64, t64, yard, what, floor=False):
    want = dict(t64, probs=p64)
    for name in NAMES:
        y = yard[name]
        if floor:
            y = max(y, 2.0 ** -24 * float(np.abs(want[name]).max()))
        ok, d = ref.within(got[name].reshape(want[name].shape), want[name], y)
        print(f'{what} {name}: device {d:.3e}, float32 restatement {yard[name]:.3e}')
        assert ok, (what, name, d, y)


def solo(net, x):
    """every tensor alone at n = 1 -> (n, 90)"""
    import torch
    d = dev(x)
    return torch.cat([net.predict(d[i:i + 1]) for i in range(len(x))]).cpu().numpy()


# ---- accuracy ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', ['counts', 'small'])
def test_accuracy_on_every_tap(net, families, expected, family):
    got = run(net, families[family])
    assert got['lstm1'].shape == (len(families[family]), 33, 256) and got['l3'].shape[1] == 7680 and got['probs'].shape[1] == 90
    check(got, *expected[family], family)
    at = 0
    for _, width in ref.HEADS:
        assert np.abs(got['probs'][:, at:at + width].sum(axis=1) - 1).max() < 1e-5
        at += width


# ---- batch and chunk edges -----------------------------------------------------------------------------------------------------------
def test_batch_edges_are_bitwise_the_tensor_alone(cn, net, families):
    x = np.concatenate([families['counts'][::2], families['small'][::2]])[:2 * cn.tile() + 3]
    alone = solo(net, x)
    t = cn.tile()
    for n in (1, t - 1, t, t + 1, 2 * t + 3):
        got = net.predict(dev(x[:n])).cpu().numpy()
        assert got.shape == (n, 90) and got.tobytes() == alone[:n].tobytes(), n
    # and a tensor does not care where in the batch it stands
    back = net.predict(dev(x[::-1])).cpu().numpy()
    assert back[::-1].tobytes() == alone.tobytes()


def test_many_tiles_are_bitwise_the_tensor_alone(cn, net, families):
    """more workgroups than CUs and the default chunk's edge: every row is still its tensor's row alone (an unordered exchange of h
    between the waves of a workgroup shows here, if anywhere, as rows that differ between copies of one tensor)"""
    x = np.concatenate([families['counts'], families['small']])
    alone = solo(net, x)
    n = net.chunk + 2 * cn.tile() + 5
    pick = np.arange(n) % len(x)
    for _ in range(2):
        got = net.predict(dev(x[pick])).cpu().numpy()
        assert got.tobytes() == alone[pick].tobytes()


def test_chunk_edges_are_bitwise_the_tensor_alone(cn, net, weights, families, monkeypatch):
    x = np.concatenate([families['counts'], families['small'], families['counts'][::-1]])[:193]
    assert len(x) == 193
    alone = solo(net, x)
    monkeypatch.setenv('MPN_CLAIR_CHUNK', '96')
    small = cn.ClairNet(weights)
    try:
        assert small.chunk == 96 and net.chunk == 4096
        for n in (95, 96, 97, 193):
            probs, taps = small.predict(dev(x[:n]), taps=True)
            assert probs.cpu().numpy().tobytes() == alone[:n].tobytes(), n
        full = net.predict(dev(x), taps=True)[1]
        for k in ref.TAPS:              # the taps of the chunks land where those of one pass do
            assert taps[k].cpu().numpy().tobytes() == full[k].cpu().numpy().tobytes(), k
    finally:
        small.close()
    monkeypatch.setenv('MPN_CLAIR_CHUNK', '0')
    with pytest.raises(ValueError, match='MPN_CLAIR_CHUNK'):
        cn.ClairNet(weights)


def test_rows_beyond_n_are_neither_read_nor_written(cn, net, families):
    import torch
    n, extra = cn.tile() + 1, 7
    x = families['small'][:n]
    want = net.predict(dev(x)).cpu().numpy()
    big = torch.full((n + extra, 33, 8, 4), 2 ** 30, dtype=torch.int32, device='cuda')
    big[:n] = dev(x)
    out = torch.full((n + extra, 90), -12345.0, dtype=torch.float32, device='cuda')
    got = net.predict(big[:n], out=out)
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert bool((out[n:] == -12345.0).all())
    # a view that does not start at the allocation's first row
    before = out.clone()
    inner = net.predict(big[3:n], out=out[5:])
    assert inner.cpu().numpy().tobytes() == want[3:].tobytes()
    assert bool((out[:5] == before[:5]).all()) and bool((out[5 + n - 3:] == before[5 + n - 3:]).all())


# ---- direction, gate order, the halves of LSTM2's kernel -----------------------------------------------------------------------------
def asymmetric_inputs(n):
    x = ref.small_inputs(n, 41)
    x[:, 20:] = 0                   # nothing in the later steps: fw and bw see different histories
    x[:, 3] += 2
    return x


def test_directions_with_time_asymmetric_inputs(net, weights):
    x = asymmetric_inputs(5)
    got = run(net, x)
    check(got, *ref.deviations(weights, x), 'asymmetric', floor=True)
    assert np.abs(got['lstm1'][:, :, :128] - got['lstm1'][:, ::-1, 128:]).max() > 1e-3


def test_one_entry_in_each_gates_column_block(cn, weights):
    w = dict(weights)
    rng = np.random.default_rng(9)
    for layer, n_in in ((1, 32), (2, 256)):
        for d in ('fw', 'bw'):
            k = np.zeros((n_in + 128, 512), dtype=np.float32)
            for gate in range(4):       # one x row and one h row per gate, at columns that differ by gate and direction
                k[int(rng.integers(0, n_in)), gate * 128 + int(rng.integers(0, 128))] = float(rng.uniform(0.2, 0.6))
                k[n_in + int(rng.integers(0, 128)), gate * 128 + int(rng.integers(0, 128))] = float(rng.uniform(0.5, 1.5))
            w[ref.CELL % (layer, d, 'kernel')] = k
            w[ref.CELL % (layer, d, 'bias')] = rng.uniform(-1, 1, size=512).astype(np.float32)
    x = ref.small_inputs(5, 42)
    sparse = cn.ClairNet(w)
    try:
        check(run(sparse, x), *ref.deviations(w, x), 'one entry per gate', floor=True)
    finally:
        sparse.close()


@pytest.mark.parametrize('zero', ['x rows', 'h rows'])
def test_lstm2_kernel_with_one_half_zero(cn, weights, zero):
    w = dict(weights)
    for d in ('fw', 'bw'):
        k = w[ref.CELL % (2, d, 'kernel')].copy()
        if zero == 'x rows':
            k[:256] = 0
        else:
            k[256:] = 0
        w[ref.CELL % (2, d, 'kernel')] = k
    x = ref.small_inputs(5, 43)
    half = cn.ClairNet(w)
    try:
        check(run(half, x), *ref.deviations(w, x), f'LSTM2 zero on its {zero}', floor=True)
    finally:
        half.close()


# ---- the layout of L3 ----------------------------------------------------------------------------------------------------------------
def test_l3_lights_exactly_one_index(cn, weights):
    w = dict(weights)
    c, u = 137, 11
    for k in range(256):
        w[f'L3/Unit_{k}/kernel'] = np.zeros((33, 30), dtype=np.float32)
        w[f'L3/Unit_{k}/bias'] = np.zeros(30, dtype=np.float32)
    one = np.zeros((33, 30), dtype=np.float32)
    one[:, u] = 0.25
    w[f'L3/Unit_{c}/kernel'] = one
    x = ref.small_inputs(3, 44)
    lit = cn.ClairNet(w)
    try:
        got = run(lit, x)
    finally:
        lit.close()
    for row in got['l3']:
        assert np.flatnonzero(row).tolist() == [u * 256 + c]
    check(got, *ref.deviations(w, x), 'one L3 unit', floor=True)


def test_two_runs_are_bit_identical(net, families):
    a, b = run(net, families['counts']), run(net, families['counts'])
    for name in NAMES:
        assert a[name].tobytes() == b[name].tobytes(), name


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def checkpoint(tmp_path_factory, weights):
    from test_clair_checkpoint import write_bundle
    prefix = str(tmp_path_factory.mktemp('clair_ckpt') / 'model-000001')
    write_bundle(prefix, weights)
    return prefix


def test_end_to_end_on_golden_bams(cn, net, weights, checkpoint, tmp_path):
    from megapath_nano_amd import clair_tensor
    resident, piped_in, n_sites, n_lines = b'', b'', 0, 0
    for name in ('iupac', 'deep_250'):
        case = tc.case_named(name)
        bam_fn, ref_fn = tc.write_case(tmp_path, case)
        kw = tc.keywords(case)
        centres, block, strings = clair_tensor.tensors(bam_fn, ref_fn, np.array(case['positions']), CTG, rng=random.Random(case['seed']), **kw)
        text = io.BytesIO()
        clair_tensor.create_tensor(bam_fn, ref_fn, np.array(case['positions']), CTG, rng=random.Random(case['seed']), out=text, **kw)
        tensor_lines = text.getvalue().decode().splitlines()
        assert len(tensor_lines) == len(centres) > 0
        out = io.BytesIO()
        n = cn.call_var_for_ensemble(net, centres, block, strings, CTG, out)
        lines = out.getvalue().decode().splitlines()
        kept = [i for i, s in enumerate(strings) if s[16] in 'ACGT']
        assert n == len(lines) == len(kept)
        if name == 'iupac':
            assert len(kept) < len(centres)          # the site with an N at its centre is absent
        p64, _, yard = ref.deviations(weights, block.cpu().numpy())
        for line, i in zip(lines, kept):
            f = line.split('\t')
            assert len(f) == 3 + 1056 + 90
            assert f[:1059] == tensor_lines[i].split()
            assert all(len(v.split('.')[1]) == 6 for v in f[1059:])
            assert np.abs(np.array(f[1059:], dtype=np.float64) - p64[i]).max() <= 4 * yard['probs'] + 0.5e-6
        resident += out.getvalue()
        piped_in += text.getvalue()
        n_sites, n_lines = n_sites + len(centres), n_lines + n
    # the tool on the piped text of both cases: the same bytes as the resident path
    p = subprocess.run([sys.executable, TOOL, '--chkpnt_fn', checkpoint, '--tensor_fn', 'PIPE', '--output_for_ensemble'], input=piped_in,
                       capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert p.stdout == resident and n_lines < n_sites


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(cn, libmpn, net, weights, families, capsys):
    import torch
    bad = dict(weights)
    bad['L5_2/kernel'] = np.zeros((192, 95), dtype=np.float32)
    with pytest.raises(ValueError, match='L5_2/kernel: shape'):
        cn.ClairNet(bad)
    flat = cn.pack_weights(weights)
    h = ct.c_void_p(None)
    assert libmpn.mpn_clair_model_create(flat.ctypes.data, len(flat) - 1, ct.byref(h)) == -2 and not h.value
    x = dev(families['small'][:4])
    for wrong in (x.to(torch.int64), x.to(torch.float32), x[:, :, :, :2], x.permute(0, 2, 1, 3), x.cpu(), x.reshape(4, 33, 32)):
        with pytest.raises(ValueError):
            net.predict(wrong)
    with pytest.raises(ValueError):
        net.predict(x, out=torch.empty((3, 90), dtype=torch.float32, device='cuda'))
    assert tuple(net.predict(x[:0]).shape) == (0, 90)
    # a freed handle
    gone = cn.ClairNet(weights)
    handle = ct.c_void_p(gone._handle.value)
    out = torch.full((4, 90), -1.0, dtype=torch.float32, device='cuda')
    gone.close()
    with pytest.raises(ValueError, match='freed'):
        gone.predict(x)
    assert libmpn.mpn_clair_forward(handle, x.data_ptr(), 4, out.data_ptr(), None) == -2
    assert libmpn.mpn_clair_model_free(handle) == -2 and libmpn.mpn_clair_model_chunk(handle) == -2
    assert bool((out == -1.0).all())
    # the command line without its only mode
    assert cn.main(['--chkpnt_fn', 'nowhere', '--tensor_fn', 'PIPE']) == 2
    assert 'only --output_for_ensemble' in capsys.readouterr().err
