"""FASTA/FASTQ ingestion for the aligner boundary (host side).

The reference hands minimap2 its target as a FIFO that `cat` fills with concatenated `.fna.gz` members
(/root/reference/bin/lib/aligner.py:143-144,209-217) or as one `.fna.gz` (:221).  A FIFO can be opened ONCE: closing the
read end makes the writer fail with EPIPE and the head of the stream is gone.  So every path is opened exactly once,
the format (saved index / BAM / gzip / plain) is sniffed from the first bytes of that one stream (`peek`, nothing consumed),
and records are parsed incrementally from it; concatenated gzip members are handled by the decompressor.

A BAM file (what ONT's basecaller writes: unaligned BAM) is read input only.  Its blocks are inflated and its records decoded on
the GPU (ingest.iter_bam_read_batches); nothing here decodes it, and a BAM given where targets are expected raises ValueError.
"""
import gzip
import io
import os
import stat
import zlib

INDEX_MAGIC = b'MPNIDX01'


def is_fifo(path):
    try:
        return stat.S_ISFIFO(os.stat(path).st_mode)
    except OSError:
        return False


def _bgzf_data_start(peeked):
    """peeked: the first bytes of a gzip stream.  -> where the deflate data of its first member starts if that member is a BGZF block
    (extra subfield BC), else 0."""
    if len(peeked) < 18 or peeked[:4] != b'\x1f\x8b\x08\x04':
        return 0
    xlen, p, found = int.from_bytes(peeked[10:12], 'little'), 12, False
    while p + 4 <= min(12 + xlen, len(peeked)):
        found |= peeked[p:p + 2] == b'BC'
        p += 4 + int.from_bytes(peeked[p + 2:p + 4], 'little')
    return 12 + xlen if found else 0


def _is_bam(peeked):
    """peeked: the first bytes of a gzip stream.  True for a BGZF block (extra subfield BC) whose text starts with BAM\\1; the first
    bytes of the block are enough to inflate those four."""
    start = _bgzf_data_start(peeked)
    if not start:
        return False
    try:
        return zlib.decompressobj(-15).decompress(peeked[start:], 4) == b'BAM\x01'
    except zlib.error:
        return False


def _open_raw(path):
    """-> (the file's own bytes as a buffered stream, opened once; its first bytes, peeked: nothing is consumed)"""
    raw = io.BufferedReader(open(path, 'rb', buffering=0), buffer_size=1 << 20)
    return raw, raw.peek(8)


def gzip_text(raw):
    """the decompressed bytes of a gzip stream (concatenated members included) from where `raw` stands"""
    return io.BufferedReader(gzip.GzipFile(fileobj=raw, mode='rb'), buffer_size=1 << 20)


def open_once(path):
    """-> (kind, binary stream); kind is 'index' (a saved mpn index: the stream is positioned at its first byte), 'bam' (the stream
    is positioned at the first byte of the file, compressed: ingest.iter_bam_read_batches takes it; told by the BAM magic at the
    start of the first BGZF block's text), 'gzip' or 'plain' (both: a stream of decompressed bytes).  The path is opened exactly once."""
    raw, peeked = _open_raw(path)
    head = peeked[:8]
    if head == INDEX_MAGIC:
        return 'index', raw
    if head[:2] == b'\x1f\x8b':
        if _is_bam(peeked):
            return 'bam', raw
        return 'gzip', gzip_text(raw)
    return 'plain', raw


def open_query(path):
    """What the read input on the device (MPN_READ_INGEST=device, ingest.iter_fastq_read_batches) wants to know of a query file:
    -> (kind, stream, first).  kind is 'index', 'bam', 'bgzf' (a gzip stream whose first member is a BGZF block, no BAM), 'gzip' or
    'plain'; the stream is ALWAYS the file's own bytes, positioned at its first byte (gzip_text decompresses it); first is the first
    byte of the text, b'' for an empty file or where the bytes at hand do not say.  The path is opened exactly once."""
    raw, peeked = _open_raw(path)
    kind, first = query_form(peeked)
    return kind, raw, first


def query_form(peeked):
    """open_query's (kind, first) from the first bytes of a file (of a stream that cannot be opened by a path: the read filter's stdin)"""
    if peeked[:8] == INDEX_MAGIC:
        return 'index', b''
    if peeked[:2] != b'\x1f\x8b':
        return 'plain', peeked[:1]
    if _is_bam(peeked):
        return 'bam', b''
    try:
        first = zlib.decompressobj(31).decompress(peeked, 1)
    except zlib.error:
        first = b''
    return ('bgzf' if _bgzf_data_start(peeked) else 'gzip'), first


def _no_bam(kind, path, what):
    if kind == 'bam':
        raise ValueError(f'{path}: a BAM file is taken as read input only, not {what}')


def iter_fastx(stream):
    """Yield (name, sequence bytes, quality bytes or None) from a binary FASTA / FASTQ stream (multi-line records, CRLF,
    mixed FASTA and FASTQ records as kseq accepts them).  The name is the first word of the header."""
    line = stream.readline()
    while line:
        line = line.rstrip(b'\r\n')
        if not line:
            line = stream.readline()
            continue
        tag = line[:1]
        if tag not in (b'>', b'@'):
            raise ValueError('neither FASTA nor FASTQ: record header expected, got %r' % line[:20])
        words = line[1:].split()
        name = words[0].decode() if words else ''
        seq = []
        line = stream.readline()
        while line and line[:1] not in (b'>', b'@', b'+'):
            seq.append(line.strip())
            line = stream.readline()
        seq = b''.join(seq)
        qual = None
        if line[:1] == b'+':
            got, parts = 0, []
            line = stream.readline()
            while line and got < len(seq):
                q = line.rstrip(b'\r\n')
                parts.append(q)
                got += len(q)
                line = stream.readline()
            qual = b''.join(parts)
            if len(qual) != len(seq):
                qual = None  # truncated quality string: kseq reports an error; the bases are still usable
        yield name, seq, qual


def read_fastx(path, with_qual=False):
    """-> list of (name, bytes) -- or (name, bytes, qual) with with_qual -- from FASTA or FASTQ, plain or gzip
    (concatenated members included), regular file or FIFO."""
    kind, stream = open_once(path)
    try:
        if kind == 'index':
            raise ValueError(f'{path}: a saved index, not sequences')
        if kind == 'bam':
            from . import ingest
            recs = ingest.read_bam(stream)
        else:
            recs = list(iter_fastx(stream))
    finally:
        stream.close()
    return recs if with_qual else [(n, s) for n, s, _ in recs]


def iter_fastx_full(stream):
    """Like iter_fastx but keeps the comment: yields (name, comment or None, sequence, quality or None)."""
    line = stream.readline()
    while line:
        line = line.rstrip(b'\r\n')
        if not line:
            line = stream.readline()
            continue
        if line[:1] not in (b'>', b'@'):
            raise ValueError('neither FASTA nor FASTQ: record header expected, got %r' % line[:20])
        head = line[1:]
        cut = len(head)
        for k, ch in enumerate(head):
            if ch in b' \t':
                cut = k
                break
        name, comment = head[:cut], (head[cut + 1:] if cut < len(head) else None)
        seq = []
        line = stream.readline()
        while line and line[:1] not in (b'>', b'@', b'+'):
            seq.append(line.strip())
            line = stream.readline()
        seq = b''.join(seq)
        qual = None
        if line[:1] == b'+':
            got, parts = 0, []
            line = stream.readline()
            while line and got < len(seq):
                q = line.rstrip(b'\r\n')
                parts.append(q)
                got += len(q)
                line = stream.readline()
            qual = b''.join(parts)
            if len(qual) != len(seq):
                qual = None
        yield name.decode(), comment, seq, qual


def subseq(in_path, names, out):
    """`seqtk subseq <in.fq> <name.lst>` (the reference writes the human/decoy-filtered reads with it,
    bin/megapath_nano.py:1221-1233): the records whose name is listed, in input order, FASTQ records as
    `@name[ comment]`, sequence, `+`, quality on single lines, FASTA records as `>name[ comment]` and the sequence.
    names: iterable of read names; out: binary stream.  -> number of records written."""
    from . import ingest
    wanted = {n if isinstance(n, str) else n.decode() for n in names}
    if ingest.read_ingest_mode() == 'device':
        kind, stream, first = open_query(in_path)
        if kind in ('plain', 'gzip', 'bgzf') and first == b'@':
            return _subseq_device(stream, kind, wanted, out)
        if kind not in ('index', 'bam'):
            stream = gzip_text(stream) if kind != 'plain' else stream        # open_once's stream: the path is opened once
    else:
        kind, stream = open_once(in_path)
    try:
        if kind == 'index':
            raise ValueError(f'{in_path}: a saved index, not sequences')
        _no_bam(kind, in_path, 'by subseq')
        return _subseq_host(stream, wanted, out)
    finally:
        stream.close()


def _subseq_host(stream, wanted, out):
    n = 0
    for name, comment, seq, qual in iter_fastx_full(stream):
        if name not in wanted:
            continue
        head = name.encode() + ((b' ' + comment) if comment is not None else b'')
        if qual is not None:
            out.write(b'@' + head + b'\n' + seq + b'\n+\n' + qual + b'\n')
        else:
            out.write(b'>' + head + b'\n' + seq + b'\n')
        n += 1
    return n


def _subseq_device(stream, kind, wanted, out, device='cuda'):
    """subseq on the text in HBM (MPN_READ_INGEST=device): per text the scan, the ids by the header rule of the read filter
    (include/mpn_ingest.h: the rule of iter_fastx_full on a plain record), and the listed records as mpn_fastq_emit writes them,
    uncropped, `@name ` keeping its blank.  From the first record the scan does not take, iter_fastx_full continues.  Closes the stream."""
    import numpy as np
    from . import fastq_filter, ingest
    n = 0
    name_set = None
    try:
        name_set = fastq_filter.NameSet([k.encode() for k in wanted])
        if kind == 'bgzf':
            texts, rest = ingest._BgzfTexts(stream, device), None
        else:
            rest = stream if kind == 'plain' else gzip_text(stream)
            texts = ingest._ChunkTexts(rest, device)
        carry = None
        while True:
            text, text_len, final = texts.next_text(carry)
            rows, consumed, status, _ = ingest.fastq_scan(text, text_len, final)
            if len(rows):
                heads, _ = fastq_filter.fastq_heads(text, text_len, rows, with_ids=False)
                keep = np.flatnonzero(fastq_filter.fastq_name_lookup(text, text_len, heads, name_set) >= 0)
                picks = np.zeros(len(keep), dtype=fastq_filter.FASTQ_PICK)
                picks['m'] = rows['len'][keep]
                picks['with_comment'] = heads['comment_len'][keep] >= 0
                d_out, out_off = fastq_filter.fastq_emit(text, text_len, rows[keep], heads[keep], picks)
                out.write(memoryview(d_out[:int(out_off[-1])].cpu().numpy()))
                n += len(keep)
            if status == ingest.FASTQ_UNSUPPORTED:
                tail = text[consumed:text_len].cpu().numpy().tobytes()
                del text, rows, carry
                return n + _subseq_host(ingest._TailThenStream(tail, rest if rest is not None else gzip_text(stream)), wanted, out)
            if status != ingest.OK:
                raise RuntimeError(f'mpn_fastq_scan: status {status}')
            if final:
                return n
            carry = text[consumed:text_len]
    finally:
        stream.close()
        if name_set is not None:
            name_set.close()


def read_split_list(path):
    """The read list of nanosplit: `read_id <whitespace> output_path` lines -> (dict name -> sorted list of output indices, output
    paths in the order of their first mention).  A pair given twice counts once.  A line without two fields raises ValueError
    (the reference tool would silently reuse the previous pair: DESIGN section 6)."""
    files, index = {}, {}
    with open(path, 'rb') as f:
        for no, raw in enumerate(f, 1):
            words = raw.split()
            if len(words) < 2:
                raise ValueError(f'{path}:{no}: a read id and an output path expected, got {raw[:40]!r}')
            name, out = words[0].decode(), os.fsdecode(words[1])
            files.setdefault(name, set()).add(index.setdefault(out, len(index)))
    return {n: sorted(s) for n, s in files.items()}, list(index)


def split_emit_plan(found, name_ptr, name_out, n_outputs, heads, rows):
    """What one scanned text contributes to the outputs of nanosplit, in numpy (no GPU).  found[r]: the list name record r is, or -1
    (fastq_filter.fastq_name_lookup); name k is listed for the outputs name_out[name_ptr[k] : name_ptr[k + 1]] (ascending); heads and
    rows: of the text's records.  -> SplitPlan: the (record, output) PAIRS sorted by (output, record) as `rec` and `out`; the emit
    `picks` of the pairs (uncropped; the comment only where it is not empty, as the reference writes it); `out_off` [pairs + 1], the
    exclusive sum of the record sizes mpn_fastq_emit checks; `pair_first` [n_outputs + 1]: output g owns the pairs
    pair_first[g] .. pair_first[g + 1], that is the bytes out_off[pair_first[g]] .. out_off[pair_first[g + 1]] of the emitted text.  A
    record whose name is listed once is one pair however often the name occurs in the text: every occurrence is its own record."""
    import collections
    import numpy as np
    from . import fastq_filter
    found, name_ptr, name_out = (np.asarray(a, dtype=np.int64) for a in (found, name_ptr, name_out))
    hit = np.flatnonzero(found >= 0)
    first = name_ptr[found[hit]]
    counts = name_ptr[found[hit] + 1] - first
    rec = np.repeat(hit, counts)
    within = np.arange(len(rec), dtype=np.int64) - np.repeat(np.cumsum(counts) - counts, counts)
    out = name_out[np.repeat(first, counts) + within]
    order = np.argsort(out, kind='stable')           # pairs arise in record order: stable by output is (output, record)
    rec, out = rec[order], out[order]
    picks = np.zeros(len(rec), dtype=fastq_filter.FASTQ_PICK)
    picks['m'] = rows['len'][rec]
    picks['with_comment'] = heads['comment_len'][rec] > 0
    out_off = np.zeros(len(rec) + 1, dtype=np.int64)
    np.cumsum(fastq_filter.record_sizes(heads[rec], picks), out=out_off[1:])
    pair_first = np.searchsorted(out, np.arange(n_outputs + 1, dtype=np.int64)).astype(np.int64)
    return collections.namedtuple('SplitPlan', 'rec out picks out_off pair_first')(rec, out, picks, out_off, pair_first)


def emit_rounds(out_off, limit):
    """Consecutive pairs of a plan in rounds of at most `limit` bytes of output and at least one pair -> [(first pair, end pair)]"""
    import numpy as np
    rounds, a, n = [], 0, len(out_off) - 1
    while a < n:
        b = max(int(np.searchsorted(out_off, out_off[a] + max(int(limit), 0), side='right')) - 1, a + 1)
        rounds.append((a, b))
        a = b
    return rounds


def _nanosplit_device(read_list_path, in_paths, device, timings):
    """nanosplit on the text in HBM (MPN_READ_INGEST=device).  One name set for the list; per input file, text by text
    (MPN_INGEST_BATCH_BYTES): the scan, the headers, mpn_fastq_name_lookup -- the ids stay on the device --, split_emit_plan, and
    mpn_fastq_emit in rounds of at most MPN_INGEST_BATCH_BYTES of output, each downloaded once and its slices appended to their
    files.  A file is open only while it is written, so the number of outputs does not meet the descriptor limit.  Texts, rounds
    and input files follow each other strictly, which is the order inside every output.  From the first record the scan does not
    take, and for an input that does not start with '@', iter_fastx_full and the host's formatting continue into the same files."""
    import time
    import numpy as np
    from . import fastq_filter, ingest
    tick = ingest._tick
    wanted, out_paths = read_split_list(read_list_path)
    for p in out_paths:
        open(p, 'wb').close()
    names = list(wanted)
    name_ptr = np.zeros(len(names) + 1, dtype=np.int64)
    np.cumsum([len(wanted[k]) for k in names], out=name_ptr[1:])
    name_out = np.array([g for k in names for g in wanted[k]], dtype=np.int64)
    counts = np.zeros(len(out_paths), dtype=np.int64)
    limit = max(1, ingest.batch_bytes())

    def append(g, data):
        with open(out_paths[g], 'ab') as f:
            f.write(data)

    def on_host(stream):
        # as the host path formats them; what is pending per output goes out at MPN_INGEST_BATCH_BYTES and at the end of the file
        t0 = time.perf_counter()
        pending, held = {}, 0
        for name, comment, seq, qual in iter_fastx_full(stream):
            groups = wanted.get(name)
            if groups is None:
                continue
            head = name.encode() + ((b' ' + comment) if comment else b'')
            rec = b'@' + head + b'\n' + seq + b'\n+\n' + qual + b'\n' if qual is not None else b'>' + head + b'\n' + seq + b'\n'
            for g in groups:
                pending.setdefault(g, []).append(rec)
                counts[g] += 1
            held += len(rec) * len(groups)
            if held > limit:
                for g in sorted(pending):
                    append(g, b''.join(pending[g]))
                pending, held = {}, 0
        for g in sorted(pending):
            append(g, b''.join(pending[g]))
        tick(timings, 'host', time.perf_counter() - t0)

    with fastq_filter.NameSet([k.encode() for k in names]) as name_set:
        for path in in_paths:
            kind, stream, first = open_query(path)
            try:
                if kind == 'index':
                    raise ValueError(f'{path}: a saved index, not sequences')
                _no_bam(kind, path, 'by nanosplit')
                if first != b'@':
                    on_host(stream if kind == 'plain' else gzip_text(stream))
                    continue
                if kind == 'bgzf':
                    texts, rest = ingest._BgzfTexts(stream, device, timings), None
                else:
                    rest = stream if kind == 'plain' else gzip_text(stream)
                    texts = ingest._ChunkTexts(rest, device, timings, 'read' if kind == 'plain' else 'inflate')
                carry = None
                while True:
                    text, text_len, final = texts.next_text(carry)
                    t0 = time.perf_counter()
                    rows, consumed, status, ms = ingest.fastq_scan(text, text_len, final)
                    t1 = time.perf_counter()
                    tick(timings, 'scan', t1 - t0)
                    tick(timings, 'scan_device_ms', ms)
                    tick(timings, 'records', len(rows))
                    if len(rows):
                        heads, _ = fastq_filter.fastq_heads(text, text_len, rows, with_ids=False)
                        t2 = time.perf_counter()
                        tick(timings, 'heads', t2 - t1)
                        tick(timings, 'heads_device_ms', fastq_filter.last_filter_device_ms()[0])
                        found = fastq_filter.fastq_name_lookup(text, text_len, heads, name_set)
                        t3 = time.perf_counter()
                        tick(timings, 'lookup', t3 - t2)
                        tick(timings, 'lookup_device_ms', fastq_filter.last_lookup_device_ms())
                        plan = split_emit_plan(found, name_ptr, name_out, len(out_paths), heads, rows)
                        tick(timings, 'plan', time.perf_counter() - t3)
                        for a, b in emit_rounds(plan.out_off, limit):
                            t4 = time.perf_counter()
                            pick = plan.rec[a:b]
                            d_out, off = fastq_filter.fastq_emit(text, text_len, rows[pick], heads[pick], plan.picks[a:b])
                            t5 = time.perf_counter()
                            tick(timings, 'emit', t5 - t4)
                            tick(timings, 'emit_device_ms', fastq_filter.last_filter_device_ms()[2])
                            written = d_out[:int(off[-1])].cpu().numpy()
                            t6 = time.perf_counter()
                            tick(timings, 'd2h', t6 - t5)
                            g = int(plan.out[a])
                            while True:        # the outputs that have pairs in [a, b), ascending
                                lo, hi = max(a, int(plan.pair_first[g])), min(b, int(plan.pair_first[g + 1]))
                                append(g, memoryview(written[int(off[lo - a]):int(off[hi - a])]))
                                counts[g] += hi - lo
                                if hi == b:
                                    break
                                g = int(plan.out[hi])
                            tick(timings, 'write', time.perf_counter() - t6)
                    if status == ingest.FASTQ_UNSUPPORTED:
                        tail = text[consumed:text_len].cpu().numpy().tobytes()
                        del text, rows, carry
                        on_host(ingest._TailThenStream(tail, rest if rest is not None else gzip_text(stream)))
                        break
                    if status != ingest.OK:
                        raise RuntimeError(f'mpn_fastq_scan: status {status}')
                    if final:
                        break
                    carry = text[consumed:text_len]
            finally:
                stream.close()
    return [(p, int(c)) for p, c in zip(out_paths, counts)]


def nanosplit(read_list_path, in_paths, device=None, timings=None):
    """The reference's bin/tools/nanosplit: every record of in_paths (FASTA / FASTQ, plain or gzip) is written to each output file
    its name is listed for, in the order of the input files and of the records in them; every listed output file is created.
    Names are expanded to record indices here; sequences and qualities are regrouped by mapper.split_reads -- on the GPU, or with
    device=False by the numpy statement of the same plan -- and the files are formatted from the group-contiguous buffers.
    Under MPN_READ_INGEST=device, unless device is False, the FASTQ text is matched and regrouped where it lies in HBM instead
    (_nanosplit_device; timings: a dict that receives its stage times); the files are the same.
    -> list of (output path, records written)"""
    from . import mapper
    if device is not False:
        from . import ingest
        if ingest.read_ingest_mode() == 'device':
            return _nanosplit_device(read_list_path, in_paths, 'cuda' if device in (None, True) else device, timings)
    wanted, out_paths = read_split_list(read_list_path)
    heads, seqs, quals, mem_read, mem_group = [], [], [], [], []
    for path in in_paths:
        kind, stream = open_once(path)
        try:
            if kind == 'index':
                raise ValueError(f'{path}: a saved index, not sequences')
            _no_bam(kind, path, 'by nanosplit')
            for name, comment, seq, qual in iter_fastx_full(stream):
                groups = wanted.get(name)
                if groups is None:
                    continue
                mem_read += [len(seqs)] * len(groups)
                mem_group += groups
                heads.append(name.encode() + ((b' ' + comment) if comment else b''))
                seqs.append(seq)
                quals.append(qual)
        finally:
            stream.close()
    packed = mapper.PackedReads([''] * len(seqs), seqs, quals=quals)
    split = mapper.split_reads(packed, mem_read, mem_group, len(out_paths), device=True if device is None else device)
    res, written = split.res, []
    for g, out_path in enumerate(out_paths):
        lo, hi = int(res['group_first'][g]), int(res['group_first'][g + 1])
        with open(out_path, 'wb') as out:
            for j in range(lo, hi):
                r, a = int(res['out_read'][j]), int(res['out_off'][j])
                b = a + int(packed.lens[r])
                if quals[r] is not None:
                    out.write(b'@' + heads[r] + b'\n' + res['seqs'][a:b].tobytes() + b'\n+\n' + res['quals'][a:b].tobytes() + b'\n')
                else:
                    out.write(b'>' + heads[r] + b'\n' + res['seqs'][a:b].tobytes() + b'\n')
        written.append((out_path, hi - lo))
    return written
