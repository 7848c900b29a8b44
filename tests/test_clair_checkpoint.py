"""CPU test: the reader of TensorFlow's tensor bundles (megapath_nano_amd/clair_net.py read_checkpoint) on the index of one of the
reference's models (tests/golden/clair_model-000016.index: names, shapes, offsets and checksums), on synthetic data files, on a tiny
bundle written here with correct checksums, and on broken files."""
import os
import shutil
import struct

import numpy as np
import pytest

from megapath_nano_amd import clair_net as cn

HERE = os.path.dirname(os.path.abspath(__file__))
INDEX = os.path.join(HERE, 'golden', 'clair_model-000016.index')
TOTAL = 11755880


def varint(v):
    out = b''
    while True:
        b = v & 0x7f
        v >>= 7
        out += bytes([b | (0x80 if v else 0)])
        if not v:
            return out


def block(entries):
    """a table block without prefix compression: every entry is a restart"""
    body, restarts = b'', []
    for key, value in entries:
        restarts.append(len(body))
        body += varint(0) + varint(len(key)) + varint(len(value)) + key + value
    return body + b''.join(struct.pack('<I', r) for r in restarts) + struct.pack('<I', len(restarts))


def write_bundle(prefix, arrays, compression=0, magic=cn.MAGIC, dtype=1, shards=1, wrong_size=False):
    data, entries = b'', [(b'', b'\x08' + varint(shards))]
    for name in sorted(arrays):
        a = np.ascontiguousarray(arrays[name], dtype='<f4')
        raw = a.tobytes()
        shape = b''.join(b'\x12' + varint(len(d)) + d for d in (b'\x08' + varint(s) for s in a.shape))
        value = b'\x08' + varint(dtype) + b'\x12' + varint(len(shape)) + shape + b'\x20' + varint(len(data)) + \
            b'\x28' + varint(len(raw) + (4 if wrong_size else 0)) + b'\x35' + struct.pack('<I', cn.mask_crc(cn.crc32c(raw)))
        entries.append((name.encode(), value))
        data += raw
    blob = b''
    data_block = block(entries)
    data_handle = varint(0) + varint(len(data_block))
    blob += data_block + bytes([compression]) + b'\0\0\0\0'
    meta_off = len(blob)
    meta = block([])
    blob += meta + b'\0' + b'\0\0\0\0'
    index_off = len(blob)
    index = block([(b'\xff', data_handle)])
    blob += index + b'\0' + b'\0\0\0\0'
    foot = varint(meta_off) + varint(len(meta)) + varint(index_off) + varint(len(index))
    blob += foot + b'\0' * (40 - len(foot)) + struct.pack('<Q', magic)
    with open(prefix + '.index', 'wb') as f:
        f.write(blob)
    with open(prefix + '.data-00000-of-00001', 'wb') as f:
        f.write(data)
    return data


@pytest.fixture(scope='module')
def synthetic(tmp_path_factory):
    d = tmp_path_factory.mktemp('clair_ckpt')
    prefix = str(d / 'model-000016')
    shutil.copyfile(INDEX, prefix + '.index')
    data = np.random.default_rng(16).integers(0, 256, size=TOTAL, dtype=np.uint8)
    data.reshape(-1, 4)[:, 3] &= 0x3f             # (no NaN patterns: the arrays compare equal to themselves)
    data.tofile(prefix + '.data-00000-of-00001')
    return prefix, data


def test_crc32c_check_value():
    assert cn.crc32c(b'123456789') == 0xE3069283
    assert cn.crc32c(b'56789', cn.crc32c(b'1234')) == 0xE3069283
    assert cn.crc32c(b'') == 0


def test_the_models_index():
    shards, entries = cn.read_index(INDEX)
    assert os.path.getsize(INDEX) == 17463 and shards == 1 and len(entries) == 540
    want = cn.variable_shapes()
    assert len(want) == 538
    for name, shape in want.items():
        assert entries[name][0] == 1 and entries[name][1] == shape, name
    assert sorted(set(entries) - set(want)) == ['LSTM1/cudnn_lstm/opaque_kernel', 'LSTM2/cudnn_lstm/opaque_kernel']
    assert entries[cn.LSTM_CELL % (1, 'fw', 'kernel')][1] == (160, 512) and entries[cn.LSTM_CELL % (2, 'bw', 'kernel')][1] == (384, 512)
    assert entries['L3/Unit_255/kernel'][1] == (33, 30) and entries['L4/kernel'][1] == (7680, 192)
    assert [entries[f'Prediction/{n}/kernel'][1] for n, _ in cn.HEADS] == [(96, 21), (96, 3), (96, 33), (96, 33)]
    at = 0
    for off, size in sorted((e[3], e[4]) for e in entries.values()):
        assert off == at
        at += size
    assert at == TOTAL
    assert cn.N_WEIGHTS == sum(int(np.prod(s)) for s in want.values()) == 2377818


def test_arrays_are_the_bytes_at_their_offsets(synthetic):
    prefix, data = synthetic
    got = cn.read_checkpoint(prefix, verify_crc=False)
    _, entries = cn.read_index(INDEX)
    assert set(got) == set(entries)
    for name, (_, shape, _, off, size, _) in entries.items():
        assert got[name].dtype == np.float32 and got[name].shape == shape
        assert got[name].tobytes() == data[off:off + size].tobytes(), name
    flat = cn.pack_weights(got)
    assert flat.dtype == np.float32 and len(flat) == cn.N_WEIGHTS
    assert np.array_equal(flat[:160 * 512], got[cn.LSTM_CELL % (1, 'fw', 'kernel')].reshape(-1))


def test_the_checksum_is_computed(synthetic):
    prefix, _ = synthetic
    with pytest.raises(ValueError, match=r'variable \S+: CRC-32C mismatch'):
        cn.read_checkpoint(prefix, verify_crc=True)


def test_a_tiny_bundle_loads_with_verification(tmp_path):
    arrays = {'a/kernel': np.arange(12, dtype=np.float32).reshape(3, 4), 'b/bias': np.array([1.5, -2.25], dtype=np.float32)}
    prefix = str(tmp_path / 'tiny')
    write_bundle(prefix, arrays)
    got = cn.read_checkpoint(prefix, verify_crc=True)
    assert sorted(got) == ['a/kernel', 'b/bias']
    assert np.array_equal(got['a/kernel'], arrays['a/kernel']) and np.array_equal(got['b/bias'], arrays['b/bias'])
    # one flipped data byte is found
    fn = prefix + '.data-00000-of-00001'
    raw = bytearray(open(fn, 'rb').read())
    raw[5] ^= 1
    open(fn, 'wb').write(bytes(raw))
    with pytest.raises(ValueError, match='a/kernel: CRC-32C mismatch'):
        cn.read_checkpoint(prefix)
    assert cn.read_checkpoint(prefix, verify_crc=False)['a/kernel'].shape == (3, 4)


def test_broken_files(tmp_path):
    arrays = {'a/kernel': np.arange(12, dtype=np.float32).reshape(3, 4), 'b/bias': np.array([1.5, -2.25], dtype=np.float32)}
    prefix = str(tmp_path / 'bad')
    write_bundle(prefix, arrays, magic=cn.MAGIC ^ 1)
    with pytest.raises(ValueError, match='bad magic at offset'):
        cn.read_checkpoint(prefix)
    write_bundle(prefix, arrays, compression=1)
    with pytest.raises(ValueError, match='offset 0 is compressed'):
        cn.read_checkpoint(prefix)
    write_bundle(prefix, arrays, dtype=3)
    with pytest.raises(ValueError, match='variable a/kernel: dtype 3 is not float'):
        cn.read_checkpoint(prefix)
    write_bundle(prefix, arrays, shards=2)
    with pytest.raises(ValueError, match='2 shards'):
        cn.read_checkpoint(prefix)
    write_bundle(prefix, arrays, wrong_size=True)
    with pytest.raises(ValueError, match=r'variable a/kernel: 52 bytes for the shape \[3, 4\]'):
        cn.read_checkpoint(prefix)
    data = write_bundle(prefix, arrays)
    with open(prefix + '.data-00000-of-00001', 'wb') as f:
        f.write(data[:-3])
    with pytest.raises(ValueError, match='variable b/bias: bytes 48 .. 56 pass the end of the file'):
        cn.read_checkpoint(prefix)


def test_pack_weights_refuses_wrong_shapes():
    w = {name: np.zeros(shape, dtype=np.float32) for name, shape in cn.variable_shapes().items()}
    assert len(cn.pack_weights(w)) == cn.N_WEIGHTS
    bad = dict(w)
    bad['L4/kernel'] = np.zeros((7680, 191), dtype=np.float32)
    with pytest.raises(ValueError, match='L4/kernel: shape'):
        cn.pack_weights(bad)
    del bad['L4/kernel']
    with pytest.raises(ValueError, match='L4/kernel is missing'):
        cn.pack_weights(bad)
