"""CPU test: the restatement of Clair's network (tests/clair_net_ref.py) is pinned against three independent statements: torch's own
bidirectional LSTM on the same weights, the slice dense written per unit as TensorFlow builds it, and the closed form of a network
with zero kernels."""
import numpy as np
import torch

import clair_net_ref as ref


def torch_lstm(w, layer, n_in):
    """torch.nn.LSTM with the weights of one layer: torch's gates are i, f, g, o, its matrices are transposed, bias_hh is 0"""
    m = torch.nn.LSTM(n_in, ref.UNITS, bidirectional=True).double()
    order = [0, 2, 1, 3]                                  # torch's block k is TensorFlow's block order[k] of i, j, f, o
    with torch.no_grad():
        for d, suffix in (('fw', ''), ('bw', '_reverse')):
            kernel = torch.as_tensor(w[ref.CELL % (layer, d, 'kernel')]).double()
            bias = torch.as_tensor(w[ref.CELL % (layer, d, 'bias')]).double()
            blocks = [kernel[:, g * ref.UNITS:(g + 1) * ref.UNITS] for g in order]
            both = torch.cat(blocks, dim=1)
            getattr(m, 'weight_ih_l0' + suffix).copy_(both[:n_in].t())
            getattr(m, 'weight_hh_l0' + suffix).copy_(both[n_in:].t())
            getattr(m, 'bias_ih_l0' + suffix).copy_(torch.cat([bias[g * ref.UNITS:(g + 1) * ref.UNITS] for g in order]))
            getattr(m, 'bias_hh_l0' + suffix).zero_()
    return m


def test_lstm_layers_equal_torchs_lstm():
    w = ref.seeded_weights(3)
    x = torch.as_tensor(ref.small_inputs(5, 1)).double().reshape(5, 33, 32).permute(1, 0, 2)
    w64 = {k: torch.as_tensor(v).double() for k, v in w.items()}
    with torch.no_grad():
        mine1 = ref.bilstm(x, w64, 1)
        theirs1, _ = torch_lstm(w, 1, 32)(x)
        assert float((mine1 - theirs1).abs().max()) <= 1e-10
        mine2 = ref.bilstm(mine1, w64, 2)
        theirs2, _ = torch_lstm(w, 2, 256)(mine1)
        assert float((mine2 - theirs2).abs().max()) <= 1e-10
    # the directions differ, and so do the layers: the comparison says something
    assert float((mine1[:, :, :128] - mine1[:, :, 128:]).abs().max()) > 1e-3
    _, taps = ref.forward(w, ref.small_inputs(5, 1))
    assert np.abs(taps['lstm1'] - mine1.permute(1, 0, 2).numpy()).max() == 0 and np.abs(taps['lstm2'] - mine2.permute(1, 0, 2).numpy()).max() == 0


def test_l3_einsum_is_the_slice_dense_as_built():
    w = {k: torch.as_tensor(v).double() for k, v in ref.seeded_weights(4).items()}
    x = torch.as_tensor(np.random.default_rng(0).standard_normal((3, 33, 256)))
    a, b = ref.l3_einsum(x, w), ref.l3_as_built(x, w)
    assert tuple(a.shape) == (3, 30, 256)
    assert float((a - b).abs().max()) <= 1e-12
    # the flattened index is u * 256 + c
    flat = a.reshape(3, 7680)
    assert float(flat[1, 7 * 256 + 5]) == float(a[1, 7, 5])


def test_zero_kernels_give_the_softmax_of_the_biases():
    w = ref.zero_weights()
    rng = np.random.default_rng(5)
    for name in w:
        if name.endswith('bias'):
            w[name] = rng.standard_normal(w[name].shape).astype(np.float32)
    probs, _ = ref.forward(w, ref.counts_inputs(3, 2))
    at = 0
    for name, width in ref.HEADS:
        bias = torch.as_tensor(w[f'Prediction/{name}/bias']).double()
        want = torch.softmax(ref.selu(bias), dim=0).numpy()
        assert np.abs(probs[:, at:at + width] - want).max() <= 1e-15
        assert abs(probs[0, at:at + width].sum() - 1) <= 1e-12
        at += width
    assert at == 90
