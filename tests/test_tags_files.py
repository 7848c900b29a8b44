"""cs / MD / =X through the outer layers: the minimap2 option spellings (AlignerOptions, bin/mpn-aligner), both BAM encoders on
=/X CIGARs and the two Z tags (CPU), and Align()'s .paf / .sam / .bam side files (-m gpu)."""
import ctypes as ct
import gzip
import os
import re
import subprocess
import sys

import pytest

from bam_reader import read_bam
from diff_tags_ref import CS, CS_LONG, EQX, MD, cigar_text, codes, collapse_eqx, parse_cigar, revcomp_codes, write_tags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- options
def test_aligner_options_accept_the_five_spellings(libmpn):
    from megapath_nano_amd.aligner import AlignerOptions
    base = ['-t', '4', '-x', 'map-ont']
    assert AlignerOptions(base, False).opt.out_tags == 0
    for args, bits in ((['--cs'], CS), (['--cs=short'], CS), (['--cs=long'], CS | CS_LONG), (['--MD'], MD), (['--eqx'], EQX),
                       (['--cs', '--MD'], CS | MD), (['--cs=long', '--eqx', '-N', '50'], CS | CS_LONG | EQX)):
        o = AlignerOptions(base + args, False)
        assert o.opt.out_tags == bits and o.opt.with_cigar == 1, (args, o.opt.out_tags)
    assert AlignerOptions(['-N', '7', '--MD', '-p', '0.5'], False).opt.best_n == 7
    assert AlignerOptions(['--cs'], True).opt.with_cigar == 0          # mapping only: kept in the options, ignored by the library
    for bad in ('--cs=foo', '--cs=', '--cs=LONG', '--md', '--eqx=1'):
        with pytest.raises(ValueError):
            AlignerOptions(base + [bad], False)


def test_map_opt_field_is_the_last_one(libmpn):
    """out_tags is appended: the offsets of the fields before it do not move, and mpn_map_opt_init clears it"""
    from megapath_nano_amd import mapper
    assert mapper.MapOpt._fields_[-1][0] == 'out_tags' and mapper.MapOpt._fields_[-2][0] == 'out_sam'
    assert mapper.MapOpt.out_tags.offset == mapper.MapOpt.out_sam.offset + 4
    o = mapper.MapOpt()
    o.out_tags = 0x7fffffff
    mapper._bind().mpn_map_opt_init(ct.byref(o))
    assert o.out_tags == 0 and o.k == 15 and o.best_n == 5
    header = open(os.path.join(ROOT, 'include', 'mpn_map.h')).read()
    for name, bit in (('MPN_TAG_CS', 1), ('MPN_TAG_CS_LONG', 2), ('MPN_TAG_MD', 4), ('MPN_TAG_EQX', 8)):
        assert re.search(r'\b%s = %d\b' % (name, bit), header), name
        assert getattr(mapper, name[4:]) == bit


def test_cli_accepts_the_options():
    exe = os.path.join(ROOT, 'bin', 'mpn-aligner')
    for args in (['--cs'], ['--cs=short'], ['--cs=long'], ['--MD'], ['--eqx'], ['-c', '--cs', '--MD', '--eqx']):
        p = subprocess.run([sys.executable, exe] + args, capture_output=True, text=True, timeout=120)
        assert p.returncode != 0 and 'unsupported option' not in p.stderr and 'usage: mpn-aligner' in p.stderr, (args, p.stderr[-500:])
    p = subprocess.run([sys.executable, exe, '--frobnicate'], capture_output=True, text=True, timeout=120)
    assert 'unsupported option --frobnicate' in p.stderr
    p = subprocess.run([sys.executable, exe, '-c', '--cs=foo', 't.fa', 'q.fq'], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and 'Traceback' not in p.stderr and 'mpn-aligner: aligner option --cs=foo' in p.stderr, p.stderr[-500:]


# -------------------------------------------------------------------------------------------------------------------- BAM
def test_both_bam_encoders_take_eqx_cigars_and_the_z_tags(libmpn, tmp_path):
    from megapath_nano_amd import bam
    lines = ['@SQ\tSN:t1\tLN:1000\n', '@SQ\tSN:t2\tLN:500\n',
             'r1\t0\tt1\t10\t60\t4=1X2I3=2D5=\t*\t0\t0\tACGTAGGACGACGTA\tIIIIIIIIIIIIIII\tNM:i:5\ttp:A:P\tcs:Z::4*ag+gg:3-tt:5\tMD:Z:4A3^TT5\trl:i:0\n',
             'r2\t16\tt2\t7\t30\t2S3=1X1=1H\t*\t0\t0\tNNACGTA\t*\tNM:i:1\tcs:Z:=ACG*tn=A\tMD:Z:3T1\trl:i:3\n',
             'r3\t2048\tt1\t300\t1\t5H6=\t*\t0\t0\tACGTAC\tIIIIII\tSA:Z:t2,1,+,5M,60,0;\tcs:Z::6\tMD:Z:6\n',
             'r4\t0\tt1\t500\t9\t3X\t*\t0\t0\tACG\tIII\tcs:Z:*ca*ac*tg\tMD:Z:0C0A0T0\n']
    sam = tmp_path / 'x.sam'
    sam.write_text(''.join(lines))
    outs = {}
    for native in (False, True):
        out = str(tmp_path / ('native.bam' if native else 'python.bam'))
        assert bam.sam_to_sorted_bam(str(sam), out, native=native) == 4
        outs[native] = out
    assert open(outs[False], 'rb').read() == open(outs[True], 'rb').read()
    # record by record, both encoders
    ref_id = {'t1': 0, 't2': 1}
    body = [l for l in lines if not l.startswith('@')]
    want = [bam.encode_record(l.rstrip('\n').split('\t'), ref_id) for l in body]
    enc = bam.NativeEncoder(['t1', 't2'])
    try:
        assert enc.encode([l.encode() for l in body]) == want
    finally:
        enc.close()
    b = read_bam(outs[True])
    by = {r['name']: r for r in b['records']}
    for l in body:
        f = l.rstrip('\n').split('\t')
        r = by[f[0]]
        assert cigar_text(r['cigar']) == f[5], f[0]
        for tag in f[11:]:
            if tag[3] == 'Z':
                assert tag[:2].encode() + b'Z' + tag[5:].encode() + b'\0' in r['aux'], (f[0], tag)
    assert [c & 15 for c in by['r1']['cigar']] == [7, 8, 1, 7, 2, 7]
    # =, X consume the reference: the end of r1 (and with it its bin and the index) counts them
    assert want[0][2] == 9 + 4 + 1 + 3 + 2 + 5


# ------------------------------------------------------------------------------------------------------ Align() side files
class FakeMetadata:
    def __init__(self, table):
        self.t = table

    def get_assembly_path(self, *, assembly_list, how='inner'):
        return assembly_list.merge(self.t[['assembly_id', 'path']].drop_duplicates(), on='assembly_id', how=how)

    def get_assembly_length(self, *, assembly_list, how='inner'):
        return assembly_list.merge(self.t[['assembly_id', 'assembly_length']].drop_duplicates(), on='assembly_id', how=how)

    def get_sequence_tax_id(self, *, assembly_list, how='inner'):
        return assembly_list.merge(self.t[['assembly_id', 'tax_id', 'species_tax_id', 'genus_tax_id', 'sequence_id']],
                                   on='assembly_id', how=how)


@pytest.mark.gpu
def test_align_side_files_carry_tags_and_eqx_cigars(libmpn, tmp_path):
    import pandas as pd
    from map_cases import small_world
    from megapath_nano_amd.aligner import Align
    d = tmp_path
    gen, reads = small_world(seed=11, n_genomes=3, glen=60000, n_reads=12, mean_len=2000)
    rows = []
    for i, (name, seq) in enumerate(gen):
        with gzip.open(d / f'asm{i}.fna.gz', 'wb') as f:
            f.write(b'>' + name.encode() + b'\n' + bytes(seq) + b'\n')
        rows.append(dict(assembly_id=f'GCF_{i:09d}.1', path=f'asm{i}.fna.gz', assembly_length=len(seq), tax_id=1000 + i,
                         species_tax_id=500 + i, genus_tax_id=50, sequence_id=name))
    with open(d / 'reads.fq', 'wb') as f:
        for r in reads:
            f.write(b'@' + r['name'].encode() + b'\n' + bytes(r['seq']) + b'\n+\n' + b'I' * len(r['seq']) + b'\n')
    table = pd.DataFrame(rows)
    common = dict(assembly_metadata=FakeMetadata(table), global_options=dict(assembly_folder=str(d), min_alignment_score=0, debug=False),
                  temp_dir_name=str(d), log_file=None, query_filename_list=pd.DataFrame({'path': [str(d / 'reads.fq')]}),
                  target_assembly_list=table[['assembly_id']].copy())
    base = ['-t', '4', '-I', '1G', '-N', '50', '-p', '1', '-x', 'map-ont', '--split-prefix', 'tmp']
    plain = Align(aligner_options=base, paf_path_and_prefix=str(d / 'plain'), **common)
    tagged = Align(aligner_options=base + ['--cs', '--MD', '--eqx'], paf_path_and_prefix=str(d / 'tagged'), **common)
    assert plain.equals(tagged)        # the table (columns only) does not change
    tcodes = {n: codes(s) for n, s in gen}
    rcodes = {r['name']: codes(r['seq']) for r in reads}
    paf, paf0 = open(d / 'tagged.paf').read(), open(d / 'plain.paf').read()
    n = 0
    for line, line0 in zip(paf.splitlines(), paf0.splitlines()):
        f, f0 = line.split('\t'), line0.split('\t')
        by = {t[:2]: t[5:] for t in f[12:]}
        if 'cg' not in by:
            assert line == line0
            continue
        assert [t[:2] for t in f[-4:]] == ['rl', 'cg', 'cs', 'MD'] and 'M' not in by['cg']
        q = rcodes[f[0]][int(f[2]):int(f[3])]
        want = write_tags(collapse_eqx(parse_cigar(by['cg'])), revcomp_codes(q) if f[4] == '-' else q, tcodes[f[5]][int(f[7]):int(f[8])])
        assert (by['cs'], by['MD'], parse_cigar(by['cg'])) == (want['cs'], want['md'], want['eqx']), f[:9]
        assert f[:-3] == f0[:-1] and cigar_text(collapse_eqx(parse_cigar(by['cg']))) == f0[-1][5:]
        n += 1
    assert n > 10 and len(paf.splitlines()) == len(paf0.splitlines())
    sam = [l.rstrip('\n').split('\t') for l in open(d / 'tagged.sam') if not l.startswith('@')]
    with_cigar = [f for f in sam if f[5] != '*']
    assert len(with_cigar) == n and all('M' not in f[5] and [t[:2] for t in f[-3:]] == ['cs', 'MD', 'rl'] for f in with_cigar)
    b = read_bam(str(d / 'tagged.bam'))
    kept = {(f[0], int(f[1]), f[2], int(f[3])): f for f in with_cigar if not int(f[1]) & 1796}
    assert len(b['records']) == len(kept) > 0
    for r in b['records']:
        f = kept[(r['name'], r['flag'], b['refs'][r['tid']][0], r['pos'] + 1)]
        assert cigar_text(r['cigar']) == f[5]
        for tag in f[11:]:
            if tag[:2] in ('cs', 'MD'):
                assert tag[:2].encode() + b'Z' + tag[5:].encode() + b'\0' in r['aux']
