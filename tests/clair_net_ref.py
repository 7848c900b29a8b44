"""A plain restatement of Clair's network (clair/model.py, structure 2BiLSTM, inference: phase=False, every dropout the identity)
in torch, written from the model's graph and not from the kernels; float64 unless asked otherwise, the layer outputs as taps.

    X (n, 33, 8, 4) -> (n, 33, 32), feature row * 4 + channel, time-major
    LSTM1, LSTM2: stack_bidirectional_dynamic_rnn of CudnnCompatibleLSTMCell(128): kernel rows [x ; h], columns i, j, f, o;
        c' = c s(f) + s(i) tanh(j), h' = tanh(c') s(o); zero state; bw over the reversed input, reversed back; concat(fw, bw)
    L3: the slice dense along the FEATURE axis: unit c takes the 33 time values of channel c to 30 values, selu; stacked on axis 2
        to (n, 30, 256), flattened with index u * 256 + c
    L4 [7680, 192] selu; L5_k [192, 96] selu, each from L4; the four heads [96, 21 | 3 | 33 | 33] selu, then a softmax each

Also what the tests of the network share: seeded weights at the initialiser's scale, the input families, and the accuracy rule."""
import numpy as np
import torch

UNITS, STEPS, FEATURES = 128, 33, 32
HEADS = (('Y_base_change_logits', 21), ('Y_genotype_logits', 3), ('Y_indel_length_logits_1', 33), ('Y_indel_length_logits_2', 33))
CELL = 'LSTM%d/stack_bidirectional_rnn/cell_0/bidirectional_rnn/%s/cudnn_compatible_lstm_cell/%s'
ALPHA, SCALE = 1.6732632423543772848170429916717, 1.0507009873554804934193349852946
TAPS = ('lstm1', 'lstm2', 'l3', 'l4')


def shapes():
    s = {}
    for layer, n_in in ((1, FEATURES), (2, 2 * UNITS)):
        for d in ('fw', 'bw'):
            s[CELL % (layer, d, 'kernel')], s[CELL % (layer, d, 'bias')] = (n_in + UNITS, 4 * UNITS), (4 * UNITS,)
    for c in range(2 * UNITS):
        s[f'L3/Unit_{c}/kernel'], s[f'L3/Unit_{c}/bias'] = (STEPS, 30), (30,)
    s['L4/kernel'], s['L4/bias'] = (7680, 192), (192,)
    for k in range(1, 5):
        s[f'L5_{k}/kernel'], s[f'L5_{k}/bias'] = (192, 96), (96,)
    for name, width in HEADS:
        s[f'Prediction/{name}/kernel'], s[f'Prediction/{name}/bias'] = (96, width), (width,)
    return s


def seeded_weights(seed, bias_scale=0.1):
    """{name: float32 array}: kernels as variance scaling with fan-in (a normal of variance 1 / inputs), random biases"""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in shapes().items():
        if name.endswith('kernel'):
            out[name] = (rng.standard_normal(shape) / np.sqrt(shape[0])).astype(np.float32)
        else:
            out[name] = (rng.standard_normal(shape) * bias_scale).astype(np.float32)
    return out


def zero_weights():
    return {name: np.zeros(shape, dtype=np.float32) for name, shape in shapes().items()}


def selu(x):
    return SCALE * torch.where(x >= 0, x, ALPHA * (torch.exp(x) - 1))


def lstm_direction(x, kernel, bias, reverse):
    """x (33, n, inputs) time-major -> (33, n, 128)"""
    steps, n = x.shape[0], x.shape[1]
    h = torch.zeros((n, UNITS), dtype=x.dtype)
    c = torch.zeros((n, UNITS), dtype=x.dtype)
    out = [None] * steps
    for t in (range(steps - 1, -1, -1) if reverse else range(steps)):
        gates = torch.cat([x[t], h], dim=1) @ kernel + bias
        i, j, f, o = torch.split(gates, UNITS, dim=1)
        c = c * torch.sigmoid(f) + torch.sigmoid(i) * torch.tanh(j)
        h = torch.tanh(c) * torch.sigmoid(o)
        out[t] = h
    return torch.stack(out)


def bilstm(x, w, layer):
    fw = lstm_direction(x, w[CELL % (layer, 'fw', 'kernel')], w[CELL % (layer, 'fw', 'bias')], False)
    bw = lstm_direction(x, w[CELL % (layer, 'bw', 'kernel')], w[CELL % (layer, 'bw', 'bias')], True)
    return torch.cat([fw, bw], dim=2)


def l3_einsum(x, w):
    """x (n, 33, 256) -> (n, 30, 256)"""
    kernel = torch.stack([w[f'L3/Unit_{c}/kernel'] for c in range(2 * UNITS)])          # (256, 33, 30)
    bias = torch.stack([w[f'L3/Unit_{c}/bias'] for c in range(2 * UNITS)])              # (256, 30)
    return selu(torch.einsum('ntc,ctu->nuc', x, kernel) + bias.t())


def l3_as_built(x, w):
    """the same as TensorFlow builds it: unstack along the feature axis, 256 dense layers, stack on axis 2"""
    sliced = torch.unbind(x, dim=2)
    return torch.stack([selu(v @ w[f'L3/Unit_{c}/kernel'] + w[f'L3/Unit_{c}/bias']) for c, v in enumerate(sliced)], dim=2)


def forward(weights, tensors, dtype=torch.float64):
    """weights {name: array}; tensors: (n, 33, 8, 4) integers -> ((n, 90) probabilities, {tap: array}) as numpy, in dtype"""
    w = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in weights.items()}
    x = torch.as_tensor(np.asarray(tensors)).to(dtype).reshape(-1, STEPS, FEATURES)
    n = x.shape[0]
    xt = x.permute(1, 0, 2)
    lstm1 = bilstm(xt, w, 1)
    lstm2 = bilstm(lstm1, w, 2)
    back = lstm2.permute(1, 0, 2)
    l3 = l3_einsum(back, w).reshape(n, 7680)
    l4 = selu(l3 @ w['L4/kernel'] + w['L4/bias'])
    probs = []
    for k, (name, _) in enumerate(HEADS, start=1):
        l5 = selu(l4 @ w[f'L5_{k}/kernel'] + w[f'L5_{k}/bias'])
        logits = selu(l5 @ w[f'Prediction/{name}/kernel'] + w[f'Prediction/{name}/bias'])
        probs.append(torch.softmax(logits, dim=1))
    taps = {'lstm1': lstm1.permute(1, 0, 2).contiguous().numpy(), 'lstm2': back.contiguous().numpy(), 'l3': l3.numpy(), 'l4': l4.numpy()}
    return torch.cat(probs, dim=1).numpy(), taps


# ---- what the tests share ------------------------------------------------------------------------------------------------------------
def golden_tensors(limit=24):
    """tensors of the tensor goldens (the lines Clair's CreateTensor.py printed), spread over the cases"""
    import tensor_cases as tc
    rows = []
    for case in tc.golden_cases():
        rows += [np.array(line.split()[3:], dtype=np.int32) for line in case['stdout'].splitlines()]
    rows = rows[::max(1, len(rows) // limit)][:limit]
    return np.stack(rows).reshape(-1, 33, 8, 4)


def counts_inputs(n, seed):
    """the saturating family: golden tensors, then random integers in [0, 100]"""
    rng = np.random.default_rng(seed)
    gold = golden_tensors(min(n // 2, 24)) if n >= 2 else np.zeros((0, 33, 8, 4), dtype=np.int32)
    rest = rng.integers(0, 101, size=(n - len(gold), 33, 8, 4)).astype(np.int32)
    return np.concatenate([gold, rest])


def small_inputs(n, seed):
    """integers in [0, 3]: the gates stay in their sensitive range"""
    return np.random.default_rng(seed).integers(0, 4, size=(n, 33, 8, 4)).astype(np.int32)


def deviations(weights, tensors):
    """The accuracy rule's two sides: the float64 values, and per tap (and 'probs') the largest absolute deviation of the restatement
    in float32 on the CPU from them -> (probs64, taps64, {name: deviation})"""
    p64, t64 = forward(weights, tensors, torch.float64)
    p32, t32 = forward(weights, tensors, torch.float32)
    dev = {k: float(np.abs(t32[k].astype(np.float64) - t64[k]).max()) for k in TAPS}
    dev['probs'] = float(np.abs(p32.astype(np.float64) - p64).max())
    return p64, t64, dev


def within(got, want64, yardstick, factor=4.0):
    """-> (ok, the deviation of `got` from the float64 values)"""
    d = float(np.abs(np.asarray(got, dtype=np.float64) - want64).max())
    return d <= factor * yardstick, d
