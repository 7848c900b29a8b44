"""Clair's network on the GPU: the consumer of the tensors of clair_tensor.py, a drop-in for what `call_var --output_for_ensemble`
computes with one model (clair/model.py, structure 2BiLSTM; inference only).  The rules and what nothing here could pin are
DESIGN.md section 6 item 18; the native calls are include/mpn_clair.h.

    read_checkpoint(prefix)                      -> {name: float32 array}: TensorFlow's tensor bundle, read without TensorFlow
    ClairNet(weights) / ClairNet.from_checkpoint -> predict(tensors): (n, 33, 8, 4) int32 on the device -> (n, 90) float32 there
    call_var_for_ensemble(net, centres, ...)     -> the lines of batch_output_for_ensemble
    bin/mpn-call-var                             the command line of the reference script (--output_for_ensemble only)

The variables go to the device once, in the one flat layout of pack_weights (= mpn_clair.h); the forward pass runs in chunks of at
most MPN_CLAIR_CHUNK tensors and leaves nothing on the host."""
import gzip
import io
import os
import struct
import sys
import ctypes as ct

import numpy as np

UNITS = 128                 # LSTM units per direction
STEPS, FEATURES = 33, 32    # time steps; 8 rows x 4 channels
L3_OUT, L4_OUT, L5_OUT = 30, 192, 96
HEADS = (('Y_base_change_logits', 21), ('Y_genotype_logits', 3), ('Y_indel_length_logits_1', 33), ('Y_indel_length_logits_2', 33))
N_PROBS = 90
LSTM_CELL = 'LSTM%d/stack_bidirectional_rnn/cell_0/bidirectional_rnn/%s/cudnn_compatible_lstm_cell/%s'
MAGIC = 0xdb4775248b80fb57
CRC_DELTA = 0xa282ead8


# ---- the checkpoint ------------------------------------------------------------------------------------------------------------------
def _crc_table():
    t = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
        t.append(c)
    # slicing by 8: eight tables, so that numpy-free Python walks a 12 MB file in a few seconds
    tables = [t]
    for k in range(1, 8):
        prev = tables[-1]
        tables.append([(prev[i] >> 8) ^ t[prev[i] & 0xff] for i in range(256)])
    return tables


_CRC = None


def crc32c(data, crc=0):
    """CRC-32C (Castagnoli) of bytes; crc: the value of the bytes before them"""
    global _CRC
    if _CRC is None:
        _CRC = _crc_table()
    t0, t1, t2, t3, t4, t5, t6, t7 = _CRC
    data = bytes(data)
    c = crc ^ 0xffffffff
    n8 = len(data) // 8
    if n8:
        for lo, hi in struct.iter_unpack('<II', data[:n8 * 8]):
            lo ^= c
            c = (t7[lo & 0xff] ^ t6[(lo >> 8) & 0xff] ^ t5[(lo >> 16) & 0xff] ^ t4[lo >> 24] ^
                 t3[hi & 0xff] ^ t2[(hi >> 8) & 0xff] ^ t1[(hi >> 16) & 0xff] ^ t0[hi >> 24])
    for b in data[n8 * 8:]:
        c = (c >> 8) ^ t0[(c ^ b) & 0xff]
    return c ^ 0xffffffff


def mask_crc(crc):
    """the form in which a tensor bundle stores a CRC"""
    return (((crc >> 15) | (crc << 17)) + CRC_DELTA) & 0xffffffff


def _varint(buf, p, what):
    v, shift = 0, 0
    while True:
        if p >= len(buf) or shift > 63:
            raise ValueError(f'{what}: a varint passes the end at offset {p}')
        b = buf[p]
        p += 1
        v |= (b & 0x7f) << shift
        if not b & 0x80:
            return v, p
        shift += 7


def _block(blob, off, size, fn):
    """the entries [(key, value)] of the table block at off"""
    if off < 0 or size < 4 or off + size + 5 > len(blob):
        raise ValueError(f'{fn}: a block at offset {off} of {size} bytes does not lie inside the file')
    if blob[off + size] != 0:
        raise ValueError(f'{fn}: the block at offset {off} is compressed (type {blob[off + size]})')
    body = blob[off:off + size]
    n_restart = struct.unpack_from('<I', body, size - 4)[0]
    end = size - 4 - 4 * n_restart
    if end < 0:
        raise ValueError(f'{fn}: the block at offset {off} has no room for its {n_restart} restarts')
    out, p, key = [], 0, b''
    while p < end:
        shared, p = _varint(body, p, fn)
        non_shared, p = _varint(body, p, fn)
        value_len, p = _varint(body, p, fn)
        if shared > len(key) or p + non_shared + value_len > end:
            raise ValueError(f'{fn}: an entry of the block at offset {off} passes its end')
        key = key[:shared] + body[p:p + non_shared]
        p += non_shared
        out.append((key, body[p:p + value_len]))
        p += value_len
    return out


def _proto(buf, what):
    """the fields of a protobuf message -> [(field, wire type, value)]"""
    out, p = [], 0
    while p < len(buf):
        tag, p = _varint(buf, p, what)
        field, wire = tag >> 3, tag & 7
        if wire == 0:
            v, p = _varint(buf, p, what)
        elif wire == 5:
            if p + 4 > len(buf):
                raise ValueError(f'{what}: a fixed32 passes the end')
            v, p = struct.unpack_from('<I', buf, p)[0], p + 4
        elif wire == 1:
            if p + 8 > len(buf):
                raise ValueError(f'{what}: a fixed64 passes the end')
            v, p = struct.unpack_from('<Q', buf, p)[0], p + 8
        elif wire == 2:
            n, p = _varint(buf, p, what)
            if p + n > len(buf):
                raise ValueError(f'{what}: a field passes the end')
            v, p = buf[p:p + n], p + n
        else:
            raise ValueError(f'{what}: wire type {wire}')
        out.append((field, wire, v))
    return out


def read_index(index_fn):
    """The table of a tensor bundle -> (num_shards, {name: (dtype, shape, shard, offset, size, masked crc)}) in key order."""
    with open(index_fn, 'rb') as f:
        blob = f.read()
    if len(blob) < 48 or struct.unpack_from('<Q', blob, len(blob) - 8)[0] != MAGIC:
        raise ValueError(f'{index_fn}: not a table: bad magic at offset {max(len(blob) - 8, 0)}')
    foot = blob[len(blob) - 48:len(blob) - 8]
    _, p = _varint(foot, 0, index_fn)
    _, p = _varint(foot, p, index_fn)           # the metaindex handle
    i_off, p = _varint(foot, p, index_fn)
    i_size, p = _varint(foot, p, index_fn)
    shards, entries = 1, {}
    for _, handle in _block(blob, i_off, i_size, index_fn):
        b_off, q = _varint(handle, 0, index_fn)
        b_size, q = _varint(handle, q, index_fn)
        for key, value in _block(blob, b_off, b_size, index_fn):
            name = key.decode()
            if name == '':
                for field, wire, v in _proto(value, f'{index_fn}: header'):
                    if field == 1 and wire == 0:
                        shards = v
                continue
            dtype, shape, shard, offset, size, crc = 0, [], 0, 0, 0, None
            for field, wire, v in _proto(value, f'{index_fn}: {name}'):
                if field == 1 and wire == 0:
                    dtype = v
                elif field == 2 and wire == 2:
                    for f2, w2, dim in _proto(v, f'{index_fn}: {name}'):
                        if f2 == 2 and w2 == 2:
                            shape += [d for f3, w3, d in _proto(dim, f'{index_fn}: {name}') if f3 == 1 and w3 == 0] or [0]
                elif field == 3 and wire == 0:
                    shard = v
                elif field == 4 and wire == 0:
                    offset = v
                elif field == 5 and wire == 0:
                    size = v
                elif field == 6 and wire == 5:
                    crc = v
            entries[name] = (dtype, tuple(shape), shard, offset, size, crc)
    return shards, entries


def read_checkpoint(prefix, verify_crc=True):
    """TensorFlow's tensor bundle prefix.index + prefix.data-00000-of-00001 -> {name: float32 array}.  ValueError, naming the
    variable or the file offset, for a bad magic, a compressed block, a dtype other than float, more than one shard, a size that
    is not 4 x the product of the shape, a data file that ends before a variable does, and (verify_crc) a CRC-32C mismatch."""
    index_fn, data_fn = prefix + '.index', prefix + '.data-00000-of-00001'
    shards, entries = read_index(index_fn)
    if shards != 1:
        raise ValueError(f'{index_fn}: {shards} shards; one is read')
    with open(data_fn, 'rb') as f:
        data = f.read()
    out = {}
    for name, (dtype, shape, shard, offset, size, crc) in entries.items():
        if dtype != 1:
            raise ValueError(f'{index_fn}: variable {name}: dtype {dtype} is not float')
        if shard != 0:
            raise ValueError(f'{index_fn}: variable {name}: shard {shard}; one is read')
        if size != 4 * int(np.prod(shape, dtype=np.int64)):
            raise ValueError(f'{index_fn}: variable {name}: {size} bytes for the shape {list(shape)}')
        if offset + size > len(data):
            raise ValueError(f'{data_fn}: variable {name}: bytes {offset} .. {offset + size} pass the end of the file ({len(data)})')
        raw = data[offset:offset + size]
        if verify_crc and (crc is None or mask_crc(crc32c(raw)) != crc):
            raise ValueError(f'{data_fn}: variable {name}: CRC-32C mismatch at offset {offset}')
        out[name] = np.frombuffer(raw, dtype='<f4').reshape(shape).copy()
    return out


# ---- the variables as the native layer takes them ------------------------------------------------------------------------------------
def variable_shapes():
    """{name: shape} of the variables the network reads, in the order of the flat layout (mpn_clair.h)"""
    shapes = {}
    for layer, n_in in ((1, FEATURES), (2, 2 * UNITS)):
        for d in ('fw', 'bw'):
            shapes[LSTM_CELL % (layer, d, 'kernel')] = (n_in + UNITS, 4 * UNITS)
            shapes[LSTM_CELL % (layer, d, 'bias')] = (4 * UNITS,)
    for c in range(2 * UNITS):
        shapes[f'L3/Unit_{c}/kernel'] = (STEPS, L3_OUT)
    for c in range(2 * UNITS):
        shapes[f'L3/Unit_{c}/bias'] = (L3_OUT,)
    shapes['L4/kernel'], shapes['L4/bias'] = (L3_OUT * 2 * UNITS, L4_OUT), (L4_OUT,)
    for k in range(1, 5):
        shapes[f'L5_{k}/kernel'], shapes[f'L5_{k}/bias'] = (L4_OUT, L5_OUT), (L5_OUT,)
    for name, width in HEADS:
        shapes[f'Prediction/{name}/kernel'], shapes[f'Prediction/{name}/bias'] = (L5_OUT, width), (width,)
    return shapes


N_WEIGHTS = sum(int(np.prod(s)) for s in variable_shapes().values())


def pack_weights(weights):
    """{name: array} -> the flat float32 array of mpn_clair_model_create.  ValueError for a missing variable or a wrong shape;
    variables the network does not read (the CudnnLSTM opaque kernels, the optimiser's) are ignored."""
    parts = []
    for name, shape in variable_shapes().items():
        if name not in weights:
            raise ValueError(f'variable {name} is missing')
        a = np.asarray(weights[name])
        if tuple(a.shape) != shape:
            raise ValueError(f'variable {name}: shape {list(a.shape)}, expected {list(shape)}')
        parts.append(np.ascontiguousarray(a, dtype=np.float32).reshape(-1))
    return np.concatenate(parts)


# ---- the native calls ----------------------------------------------------------------------------------------------------------------
_bound = False


def _lib():
    global _bound
    from . import candidates
    lib = candidates._lib()
    if not _bound:
        P, I64, I32 = ct.c_void_p, ct.c_int64, ct.c_int32
        lib.mpn_clair_model_create.argtypes = [P, I64, ct.POINTER(P)]
        lib.mpn_clair_model_free.argtypes = [P]
        lib.mpn_clair_forward.argtypes = [P, P, I64, P, P]
        lib.mpn_clair_model_chunk.argtypes = [P]
        lib.mpn_clair_tile.argtypes = []
        for f in (lib.mpn_clair_model_create, lib.mpn_clair_model_free, lib.mpn_clair_forward, lib.mpn_clair_tile):
            f.restype = I32
        lib.mpn_clair_model_chunk.restype = I64
        lib.mpn_clair_last_device_ms.argtypes = [ct.POINTER(ct.c_double)] * 6
        lib.mpn_clair_last_device_ms.restype = None
        _bound = True
    return lib


def _check(rc, what):
    """-2 (bad arguments) is a ValueError, anything else the native layer's error"""
    from . import _ffi
    if rc == -2:
        raise ValueError(f'{what}: {_ffi.last_error()}')
    if rc:
        raise _ffi.MpnError(f'{what} rc={rc}: {_ffi.hint(_ffi.last_error())}')


STAGES = ('project_ms', 'recurrent_ms', 'l3_ms', 'l4_ms', 'heads_ms', 'total_ms')


def last_device_ms():
    """-> {stage: device ms} of the calling thread's last forward: the two input projections, the two recurrent passes, L3, L4, the
    small layers with the softmaxes, and everything (tap copies included)"""
    v = [ct.c_double(0) for _ in range(6)]
    _lib().mpn_clair_last_device_ms(*[ct.byref(x) for x in v])
    return dict(zip(STAGES, (x.value for x in v)))


def tile():
    """MPN_CLAIR_TILE: the batch rows one workgroup of the recurrent kernel carries"""
    return int(_lib().mpn_clair_tile())


class _Taps(ct.Structure):          # mpn_clair_taps
    _fields_ = [('lstm1', ct.c_void_p), ('lstm2', ct.c_void_p), ('l3', ct.c_void_p), ('l4', ct.c_void_p)]


class ClairNet:
    """The network with its variables on the device.  weights: {name: array} as read_checkpoint gives them."""

    def __init__(self, weights, device='cuda'):
        self._handle = None
        flat = pack_weights(weights)
        self.device = device
        h = ct.c_void_p(None)
        _check(_lib().mpn_clair_model_create(flat.ctypes.data, len(flat), ct.byref(h)), 'mpn_clair_model_create')
        self._handle = h

    @classmethod
    def from_checkpoint(cls, prefix, device='cuda', verify_crc=True):
        return cls(read_checkpoint(prefix, verify_crc), device)

    @property
    def chunk(self):
        """the tensors of one pass (MPN_CLAIR_CHUNK when the model was made)"""
        self._live()
        return int(_lib().mpn_clair_model_chunk(self._handle))

    def _live(self):
        if self._handle is None:
            raise ValueError('the model has been freed')

    def close(self):
        if self._handle is not None:
            _lib().mpn_clair_model_free(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def predict(self, tensors, taps=False, out=None):
        """tensors: an (n, 33, 8, 4) or (n, 1056) int32 tensor on the device, contiguous -> an (n, 90) float32 tensor there:
        gt21 | genotype | length_1 | length_2.  taps: also {'lstm1': (n, 33, 256), 'lstm2': (n, 33, 256), 'l3': (n, 7680),
        'l4': (n, 192)}.  out: a contiguous float32 tensor whose first n rows are written.  ValueError for anything else."""
        import torch
        self._live()
        if not isinstance(tensors, torch.Tensor) or tensors.dtype != torch.int32 or not tensors.is_cuda:
            raise ValueError('the tensors are not an int32 tensor on the device')
        if not tensors.is_contiguous() or tensors.dim() < 1 or (tensors.numel() and tuple(tensors.shape[1:]) not in ((33, 8, 4), (1056,))):
            raise ValueError(f'the tensors are not a contiguous (n, 33, 8, 4) block: shape {list(tensors.shape)}')
        n = tensors.shape[0]
        if out is None:
            out = torch.empty((n, N_PROBS), dtype=torch.float32, device=tensors.device)
        elif out.dtype != torch.float32 or not out.is_contiguous() or out.dim() != 2 or out.shape[1] != N_PROBS or out.shape[0] < n or not out.is_cuda:
            raise ValueError('the output is not a contiguous (>= n, 90) float32 tensor on the device')
        tp, got = None, None
        if taps:
            got = {'lstm1': torch.empty((n, STEPS, 2 * UNITS), dtype=torch.float32, device=tensors.device),
                   'lstm2': torch.empty((n, STEPS, 2 * UNITS), dtype=torch.float32, device=tensors.device),
                   'l3': torch.empty((n, L3_OUT * 2 * UNITS), dtype=torch.float32, device=tensors.device),
                   'l4': torch.empty((n, L4_OUT), dtype=torch.float32, device=tensors.device)}
            tp = _Taps(*[got[k].data_ptr() if n else None for k in ('lstm1', 'lstm2', 'l3', 'l4')])
        if n:
            torch.cuda.current_stream(tensors.device).synchronize()         # the native layer uses the default stream
            _check(_lib().mpn_clair_forward(self._handle, tensors.data_ptr(), n, out.data_ptr(), ct.byref(tp) if tp is not None else None),
                              'mpn_clair_forward')
        probs = out[:n]
        return (probs, got) if taps else probs


# ---- the lines -----------------------------------------------------------------------------------------------------------------------
def call_var_for_ensemble(net, centres, tensors, refs, ctg_name, out):
    """The lines of call_var's batch_output_for_ensemble for one model: chrom, pos, refseq, the 1056 integers and the 90
    probabilities as %.6f, tab-separated.  centres: the 1-based position (or its text) per tensor; refs: the reference string per
    tensor; a site whose centre base (index 16) is not one of ACGT is skipped.  out: a binary stream -> the number of lines."""
    probs = net.predict(tensors).cpu().numpy()
    cells = tensors.reshape(len(probs), -1).cpu().numpy()
    n = 0
    for pos, seq, x, p in zip(centres, refs, cells, probs):
        if len(seq) <= 16 or seq[16] not in 'ACGT':
            continue
        out.write('\t'.join([ctg_name, str(pos), seq] + [str(v) for v in x.tolist()] + ['%.6f' % v for v in p.tolist()]).encode() + b'\n')
        n += 1
    return n


def read_tensor_lines(stream):
    """the lines of mpn-create-tensor (`ctg pos refseq t0 .. t1055`) -> [(ctg, pos text, refseq)], an (n, 1056) int32 array"""
    heads, rows = [], []
    for line in stream:
        f = line.split()
        if not f:
            continue
        if len(f) != 3 + 1056:
            raise ValueError(f'a tensor line has {len(f)} columns, not 1059')
        heads.append(tuple(x.decode() if isinstance(x, bytes) else x for x in f[:3]))
        rows.append(np.array(f[3:], dtype=np.int32))
    return heads, (np.stack(rows) if rows else np.zeros((0, 1056), dtype=np.int32))


def main(argv, prog='mpn-call-var'):
    """The command line of clair/call_var.py, for --output_for_ensemble."""
    from argparse import ArgumentParser
    ap = ArgumentParser(prog=prog, description='Probabilities of Clair\'s network for tensors, one model, for the ensemble (on the GPU)')
    ap.add_argument('--chkpnt_fn', type=str, default=None, help='the prefix of a model checkpoint (prefix.index, prefix.data-00000-of-00001)')
    ap.add_argument('--tensor_fn', type=str, default='PIPE', help='Tensor input of mpn-create-tensor: a gzip file, PIPE for standard input')
    ap.add_argument('--call_fn', type=str, default=None, help='Output file; standard output when not given')
    ap.add_argument('--output_for_ensemble', action='store_true', help='Output the probabilities for the ensemble (the only mode)')
    ap.add_argument('--no_crc', action='store_true', help='do not verify the checkpoint\'s checksums')
    if not argv:
        ap.print_help()
        return 1
    a = ap.parse_args(argv)
    if not a.output_for_ensemble:
        print(f'{prog}: only --output_for_ensemble is implemented: the VCF decoding of call_var is not part of this tool', file=sys.stderr)
        return 2
    if not a.chkpnt_fn:
        print(f'{prog}: --chkpnt_fn is needed', file=sys.stderr)
        return 2
    try:
        import torch
        net = ClairNet.from_checkpoint(a.chkpnt_fn, verify_crc=not a.no_crc)
        if a.tensor_fn == 'PIPE':
            heads, cells = read_tensor_lines(sys.stdin.buffer)
        else:
            with gzip.open(a.tensor_fn, 'rb') as f:
                heads, cells = read_tensor_lines(f)
        buf = io.BytesIO()
        at = 0
        while at < len(heads):       # a contig at a time, as the lines name it
            b = at
            while b < len(heads) and heads[b][0] == heads[at][0]:
                b += 1
            block = torch.from_numpy(cells[at:b]).to(net.device).reshape(-1, 33, 8, 4)
            call_var_for_ensemble(net, [h[1] for h in heads[at:b]], block, [h[2] for h in heads[at:b]], heads[at][0], buf)
            at = b
    except (ValueError, OSError) as e:
        print(f'{prog}: {e}', file=sys.stderr)
        return 1
    if a.call_fn:
        os.makedirs(os.path.dirname(os.path.abspath(a.call_fn)), exist_ok=True)
        with open(a.call_fn, 'wb') as f:
            f.write(buf.getvalue())
    else:
        sys.stdout.buffer.write(buf.getvalue())
        sys.stdout.buffer.flush()
    return 0
