"""GPU tests (-m gpu) of the FASTQ scan and gather (include/mpn_ingest.h: mpn_fastq_scan, mpn_fastq_gather): the device against the
restatement tests/fastq_scan_ref.py row for row, and the gathered bytes and names against fastx.iter_fastx, on the texts of
fastq_scan_ref (tests/test_fastq_scan_ref.py holds the restatement itself against iter_fastx, without a GPU)."""
import ctypes as ct

import numpy as np
import pytest

import fastq_scan_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def tile(libmpn):
    from megapath_nano_amd import ingest
    t = ingest.fastq_tile()
    assert t == ref.header_tile()
    return t


def upload(data, shift=0):
    """the bytes in HBM, `shift` bytes into a 16-byte aligned buffer; behind them a sentinel the scan must not take for text"""
    import torch
    buf = np.full(shift + len(data) + 64, ord('@'), dtype=np.uint8)
    buf[shift:shift + len(data)] = np.frombuffer(data, dtype=np.uint8)
    return torch.from_numpy(buf).cuda()[shift:]


def scan(text, final, shift=0, rec_cap=None):
    from megapath_nano_amd import ingest
    rows, consumed, status, _ = ingest.fastq_scan(upload(text, shift), len(text), final, rec_cap=rec_cap)
    return rows, consumed, status


def tuples(rows):
    return [tuple(int(x) for x in r) for r in rows.tolist()]


def check_against_ref(text, final, shift=0):
    want_rows, want_consumed, want_status = ref.scan(text, final)
    rows, consumed, status = scan(text, final, shift)
    assert (consumed, status) == (want_consumed, want_status)
    assert tuples(rows) == tuples(want_rows)
    return rows, consumed, status


def gathered(text, rows):
    """[(name, bases, qualities)] of the rows through mpn_fastq_gather"""
    from megapath_nano_amd import ingest
    seq, qual, names = ingest.fastq_gather(upload(text), len(text), rows)
    seq, qual = seq.cpu().numpy(), qual.cpu().numpy()
    lens = rows['len'].astype(np.int64)
    off = np.cumsum(lens) - lens
    total = int(lens.sum())
    assert len(seq) == len(qual) == (total + 16 + 15) // 16 * 16
    assert not seq[total:].any() and not qual[total:].any()
    return [(names[i], seq[off[i]:off[i] + lens[i]].tobytes(), qual[off[i]:off[i] + lens[i]].tobytes()) for i in range(len(rows))]


# ---- the scan ---------------------------------------------------------------------------------------------------------------------
def _plain_groups(tile):
    cases = ref.plain_cases(tile)
    groups = {'edges1': [c for c in cases if c[0].startswith('edge1')], 'edges2': [c for c in cases if c[0].startswith('edge2')]}
    for c in cases:
        if not c[0].startswith('edge'):
            groups[c[0]] = [c]
    return groups


GROUPS = sorted(_plain_groups(ref.header_tile()))


@pytest.mark.parametrize('group', GROUPS)
def test_plain_texts_equal_the_restatement_and_iter_fastx(tile, group):
    for name, text, final in _plain_groups(tile)[group]:
        rows, consumed, status = check_against_ref(text, final)
        assert status == ref.OK, name
        assert gathered(text, rows) == ref.host_records(text[:consumed]), name
        if final:
            assert consumed == len(text) and len(rows) == len(ref.host_records(text)), name


@pytest.mark.parametrize('shift', [1, 7, 15])
def test_text_at_any_alignment(tile, shift):
    cases = {c[0]: c for c in ref.plain_cases(tile)}
    for name in ('long_reads', 'crlf', 'edge1_+1_line3', 'no_last_lf_final'):
        _, text, final = cases[name]
        check_against_ref(text, final, shift)


def test_table_one_too_small_then_the_counting_call(tile):
    from megapath_nano_amd import _ffi, ingest
    _, text, _ = next(c for c in ref.plain_cases(tile) if c[0] == 'short_3000')
    lib, d_text = ingest._lib(), upload(text)
    rows = np.zeros(2999, dtype=ingest.FASTQ_ROW)
    n, consumed, status = ct.c_int64(-1), ct.c_int64(-1), ct.c_int32(-1)
    rc = lib.mpn_fastq_scan(d_text.data_ptr(), len(text), 1, 2999, rows.ctypes.data, ct.byref(n), ct.byref(consumed), ct.byref(status))
    assert rc == -3 and (n.value, consumed.value, status.value) == (3000, len(text), ref.OK), _ffi.last_error()
    n, consumed, status = ct.c_int64(-1), ct.c_int64(-1), ct.c_int32(-1)
    rc = lib.mpn_fastq_scan(d_text.data_ptr(), len(text), 1, 0, None, ct.byref(n), ct.byref(consumed), ct.byref(status))
    assert rc == 0 and (n.value, consumed.value, status.value) == (3000, len(text), ref.OK)
    # the wrapper makes the table again when its guess was too small
    got, _, _ = scan(text, True, rec_cap=1)
    assert tuples(got) == tuples(ref.scan(text, True)[0])


def test_cuts_without_final_resume_with_the_carried_tail():
    for name, text, cut in ref.cut_cases():
        whole = ref.scan(text, True)[0]
        rows, consumed, status = check_against_ref(text[:cut], False)
        assert status == ref.OK, name
        ends = [0] + [int(w['qual_off']) + int(w['len']) + 1 for w in whole]
        assert consumed == max(e for e in ends if e <= cut), name
        rest, consumed2, status2 = check_against_ref(text[consumed:], True)
        assert status2 == ref.OK and consumed + consumed2 == len(text), name
        assert gathered(text[:cut], rows) + gathered(text[consumed:], rest) == ref.host_records(text), name


def test_every_reason_for_unsupported():
    for name, text, final, before in ref.unsupported_cases():
        rows, consumed, status = check_against_ref(text, final)
        assert status == ref.UNSUPPORTED and len(rows) == before, name
        assert consumed == sum(len(g) for g in ref.GOOD[:before]), name
        assert gathered(text, rows) + ref.host_records(text[consumed:]) == ref.host_records(text), name
    for name, bad in ref.TRUNCATED:        # the same cut short without final: carried, not refused
        rows, consumed, status = check_against_ref(ref.GOOD[0] + bad, False)
        assert (len(rows), consumed, status) == (1, len(ref.GOOD[0]), ref.OK), name


def test_htslib_files():
    for name, text, want in ref.htslib_cases():
        rows, consumed, status = check_against_ref(text, True)
        if want is None:
            assert status == ref.OK and consumed == len(text), name
            assert gathered(text, rows) == ref.host_records(text), name
        else:                               # multi-line records: the host reads the file
            assert status == ref.UNSUPPORTED and len(rows) == want, name


# ---- the gather -------------------------------------------------------------------------------------------------------------------
def test_gather_of_a_subset_in_another_order(tile):
    _, text, _ = next(c for c in ref.plain_cases(tile) if c[0] == 'long_reads')
    text = text + next(c for c in ref.plain_cases(tile) if c[0] == 'short_3000')[1]
    rows = ref.scan(text, True)[0]
    recs = ref.records(text, rows)
    pick = np.array([3, 0, 4, 2, 2, 1] + list(range(3004, 4, -7)))
    assert gathered(text, rows[pick]) == [recs[i] for i in pick]


def test_gather_changes_only_the_promised_bytes():
    import torch
    from megapath_nano_amd import ingest
    text = b''.join(ref.GOOD)
    rows = ref.scan(text, True)[0]
    lens = rows['len'].astype(np.int64)
    off = np.ascontiguousarray(np.cumsum(lens) - lens)
    total = int(lens.sum())
    size = (total + 16 + 15) // 16 * 16
    lib, d_text = ingest._lib(), upload(text)
    seq = torch.full((64 + size + 64,), 0xA5, dtype=torch.uint8, device='cuda')
    qual = torch.full((64 + size + 64,), 0x5A, dtype=torch.uint8, device='cuda')
    pool = np.full(int(rows['name_len'].sum()) + 8, 0x7E, dtype=np.uint8)
    rc = lib.mpn_fastq_gather(d_text.data_ptr(), len(text), len(rows), rows.ctypes.data, off.ctypes.data, seq.data_ptr() + 64, qual.data_ptr() + 64,
                              pool.ctypes.data, pool.size - 8)
    assert rc == 0
    seq, qual = seq.cpu().numpy(), qual.cpu().numpy()
    assert (seq[:64] == 0xA5).all() and (seq[64 + size:] == 0xA5).all() and (qual[:64] == 0x5A).all() and (qual[64 + size:] == 0x5A).all()
    recs = ref.records(text, rows)
    assert seq[64:64 + total].tobytes() == b''.join(r[1] for r in recs) and qual[64:64 + total].tobytes() == b''.join(r[2] for r in recs)
    assert not seq[64 + total:64 + size].any() and not qual[64 + total:64 + size].any() and size - total >= 16
    assert pool[:-8].tobytes() == ''.join(r[0] for r in recs).encode() and (pool[-8:] == 0x7E).all()
    # without qualities; a pool that is too small; no rows at all
    seq2 = torch.full((size,), 0xA5, dtype=torch.uint8, device='cuda')
    assert lib.mpn_fastq_gather(d_text.data_ptr(), len(text), len(rows), rows.ctypes.data, off.ctypes.data, seq2.data_ptr(), None, pool.ctypes.data,
                                pool.size) == 0
    assert seq2.cpu().numpy().tobytes() == seq[64:64 + size].tobytes()
    assert lib.mpn_fastq_gather(d_text.data_ptr(), len(text), len(rows), rows.ctypes.data, off.ctypes.data, seq2.data_ptr(), None, pool.ctypes.data,
                                1) == -3
    seq3 = torch.full((32,), 0xA5, dtype=torch.uint8, device='cuda')
    assert lib.mpn_fastq_gather(d_text.data_ptr(), len(text), 0, None, None, seq3.data_ptr(), None, None, 0) == 0
    assert seq3.cpu().numpy().tolist() == [0] * 16 + [0xA5] * 16


def test_gather_refuses_rows_outside_the_text():
    import torch
    from megapath_nano_amd import ingest
    text = b''.join(ref.GOOD)
    good = ref.scan(text, True)[0]
    lens = good['len'].astype(np.int64)
    off = np.ascontiguousarray(np.cumsum(lens) - lens)
    lib, d_text = ingest._lib(), upload(text)
    seq = torch.full((256,), 0xA5, dtype=torch.uint8, device='cuda')
    pool = np.zeros(64, dtype=np.uint8)

    def call(rows, offs=off, text_len=len(text)):
        rows = np.ascontiguousarray(rows)
        return lib.mpn_fastq_gather(d_text.data_ptr(), text_len, len(rows), rows.ctypes.data, offs.ctypes.data, seq.data_ptr(), None, pool.ctypes.data,
                                    pool.size)
    assert call(good) == 0
    assert call(good, text_len=len(text) - 2) == -2                 # the last row's qualities pass text_len
    for field, value in (('seq_off', len(text) - 3), ('qual_off', len(text)), ('qual_off', -1), ('seq_off', -1), ('name_off', len(text)),
                         ('len', -1), ('name_len', -1), ('seq_off', 1 << 62)):
        rows = good.copy()
        rows[field][1] = value
        assert call(rows) == -2, (field, value)
    rows = good.copy()
    rows['len'][0] += 1                                             # out_off is no longer the exclusive sum
    assert call(rows) == -2
    assert (seq.cpu().numpy()[64:] == 0xA5).all()
