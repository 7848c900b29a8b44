"""GPU tests (-m gpu) of mpn_fasta_scan (csrc/fasta_kernels.hip) against fastx.iter_fastx, which defines the records: every
stream's names, lengths and bases must be what iter_fastx yields for the same bytes read as one file.  A tile is 4096 bytes."""
import io

import numpy as np
import pytest

from megapath_nano_amd import fastx

pytestmark = pytest.mark.gpu
TILE = 4096
OK, UNSUPPORTED = 0, 9
GAP = b'\n>GAP\nQQ'     # between the streams in the text buffer: a scan that leaves its stream meets a record that is not there


@pytest.fixture(scope='module')
def ingest(libmpn):
    from megapath_nano_amd import ingest
    return ingest


def host_records(stream):
    return [(n, s) for n, s, _ in fastx.iter_fastx(io.BytesIO(stream))]


def scan(ingest, streams):
    import torch
    off, text = [], b''
    for s in streams:
        text += GAP
        off.append(len(text))
        text += s
    text += GAP
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to('cuda')
    res = ingest.scan_fasta(d_text, np.array(off, dtype=np.int64), np.array([len(s) for s in streams], dtype=np.int64))
    bases = res.seq[res.seq_pos:res.seq_pos + int(res.n_bases.sum())].cpu().numpy().tobytes()
    return res, bases


def check_equal(ingest, streams):
    res, bases = scan(ingest, streams)
    want = [host_records(s) for s in streams]
    assert res.status.tolist() == [OK] * len(streams)
    assert res.n_records.tolist() == [len(w) for w in want]
    assert res.n_bases.tolist() == [sum(len(s) for _, s in w) for w in want]
    flat = [(k, n, s) for k, w in enumerate(want) for n, s in w]
    assert res.stream.tolist() == [k for k, _, _ in flat]
    assert res.names == [n for _, n, _ in flat]
    assert res.lens.tolist() == [len(s) for _, _, s in flat]
    assert bases == b''.join(s for _, _, s in flat)
    return res


def seq(rng, n, alphabet=b'ACGT'):
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), size=n)].tobytes()


def wrap(s, width=80, eol=b'\n'):
    return b''.join(s[a:a + width] + eol for a in range(0, len(s), width))


def test_line_ends_blank_lines_and_stream_ends(ingest):
    rng = np.random.default_rng(1)
    streams = [
        b'>crlf one\r\n' + wrap(seq(rng, 500), 60, b'\r\n') + b'>crlf2\r\n' + wrap(seq(rng, 130), 60, b'\r\n'),
        b'\n\n>blank lines\n\n' + seq(rng, 70) + b'\n\n\r\n' + seq(rng, 70) + b'\n\n>second\n\n\n' + seq(rng, 10) + b'\n\n',
        b'>no final newline\n' + seq(rng, 100),                       # must not glue onto the next stream's first line
        b'>after it\n' + seq(rng, 50) + b'\n',
        b'>ends in a header\n' + seq(rng, 33) + b'\n>header only',
        b'',
        b'>trailing cr\n' + seq(rng, 20) + b'\r',
        b'\n',
    ]
    check_equal(ingest, streams)


def test_names_and_sequence_bytes(ingest):
    rng = np.random.default_rng(2)
    streams = [
        b'>header_only_in_the_middle\n>next words here\n' + seq(rng, 90) + b'\n',
        b'>\n' + seq(rng, 40) + b'\n> description without a name\n' + seq(rng, 41) + b'\n>\r\n' + seq(rng, 5) + b'\n',
        b'>gt\nAC>GT>\nAA>\n>real\tname\nA\n',                         # '>' inside a line is a sequence byte
        b'>  spaced   name\n' + seq(rng, 30) + b'\n>tab\tafter\n' + seq(rng, 30) + b'\n>cr\rinside\n' + seq(rng, 7) + b'\n',
        b'>lower and iupac\n' + wrap(seq(rng, 1000, b'acgtnACGTNRYKMSWBDHVryk-*.')) + b'>N\nNNNNNNNNNN\n',
    ]
    check_equal(ingest, streams)


def test_lines_longer_than_a_tile(ingest):
    rng = np.random.default_rng(3)
    long_header = b'>' + b'n' * 30 + b' ' + b'd' * 70_000
    streams = [
        b'>long_line\n' + seq(rng, 70_000) + b'\n>after\n' + seq(rng, 100) + b'\n',
        long_header + b'\n' + seq(rng, 200) + b'\n>x\n' + seq(rng, 9000) + b'\n',
        b'>' + b'w' * 70_000 + b'\nACGT\n',                                  # a name longer than a tile
        b'>unwrapped_no_newline\n' + seq(rng, 70_001),
    ]
    check_equal(ingest, streams)


def test_record_starts_around_a_tile_edge(ingest):
    rng = np.random.default_rng(4)
    streams = []
    for edge in (TILE, 2 * TILE):
        for d in (-2, -1, 0, 1, 2):
            head = b'>a\n'
            body = seq(rng, edge + d - len(head) - 1) + b'\n'              # the '>' of the second record lands on byte edge + d
            s = head + body + b'>b%d\n' % d + seq(rng, 50) + b'\n'
            assert s[edge + d:edge + d + 1] == b'>' and s[edge + d - 1:edge + d] == b'\n'
            streams.append(s)
            streams.append(head + wrap(seq(rng, edge), 80)[:edge + d - len(head) - 1] + b'\n>c\n' + seq(rng, 5))   # wrapped lines up to the edge
    check_equal(ingest, streams)


def test_many_streams_in_one_call(ingest):
    rng = np.random.default_rng(5)
    streams = []
    for k in range(300):
        s = b''
        for r in range(int(rng.integers(1, 4))):
            s += b'>s%d_r%d some text\n' % (k, r) + wrap(seq(rng, int(rng.integers(0, 9000))), 80)
        streams.append(s if k % 7 else s.rstrip(b'\n'))
    res = check_equal(ingest, streams)
    assert 300 <= len(res.names) <= 900


def test_unsupported_streams_are_flagged_and_their_neighbours_are_not(ingest):
    rng = np.random.default_rng(6)
    good = b'>good\n' + wrap(seq(rng, 5000))
    flagged = [
        b'ACGT\n>late header\nACGT\n',                      # the first non-blank line is not a header
        b'\n\n  \n>x\nACGT\n',                               # (a line of blanks is not blank to iter_fastx either)
        b'>q\nACGT\n@read\nACGT\n+\nIIII\n',                # FASTQ
        b'>q\nACGT\n+\n',
        b'>q\nAC GT\n',                                     # the host strips these per line
        b'>q\nACGT\t\n',
        b'>q\n\x0bACGT\n',
        b'>q\nACGT\x0c\n',
        b'>q\nAC\rGT\n',                                    # a CR that is no line end stays in the host's sequence
        seq(rng, 9000),                                     # no header at all, more than a tile
    ]
    streams = []
    for f in flagged:
        streams += [good, f]
    streams.append(good)
    res, _ = scan(ingest, streams)
    assert res.status.tolist() == [OK, UNSUPPORTED] * len(flagged) + [OK]
    assert [int(res.n_records[k]) for k in range(0, len(streams), 2)] == [1] * (len(flagged) + 1)
    assert [int(res.n_bases[k]) for k in range(0, len(streams), 2)] == [5000] * (len(flagged) + 1)


def test_bases_land_behind_out_pos(ingest):
    import torch
    rng = np.random.default_rng(7)
    s = b'>a\n' + wrap(seq(rng, 10_000))
    d_text = torch.frombuffer(bytearray(s), dtype=torch.uint8).to('cuda')
    out = torch.full((10_000 + 77 + 33,), 0x5A, dtype=torch.uint8, device='cuda')
    res = ingest.scan_fasta(d_text, np.array([0]), np.array([len(s)]), out=out, out_pos=77)
    got = out.cpu().numpy().tobytes()
    assert got[:77] == b'\x5a' * 77 and got[77 + 10_000:] == b'\x5a' * 33
    assert got[77:77 + 10_000] == host_records(s)[0][1] and res.lens.tolist() == [10_000]
