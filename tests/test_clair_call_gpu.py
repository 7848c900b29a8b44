"""GPU tests (-m gpu) of the decoding of Clair's probabilities (megapath_nano_amd/clair_call.py, csrc/clair_call_kernels.hip) against
the restatement (tests/clair_call_ref.py in 'legacy'): every line byte for byte, every row integer- and bit-exact."""
import io
import os
import random
import struct
import subprocess
import sys

import numpy as np
import pytest

import clair_call_cases as cc
import clair_call_ref as ref
import pileup_cases as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'bin', 'mpn-call-vcf')


@pytest.fixture(scope='module')
def call(libmpn):
    from megapath_nano_amd import clair_call
    return clair_call


def files(tmp_path, case):
    d = str(tmp_path)
    return (pc.write_bam(os.path.join(d, 'in.bam'), [(cc.CTG, case['seq'])], case['lines']), pc.write_fasta(os.path.join(d, 'ref.fa'), [(cc.CTG, case['seq'])]))


def dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def lines_of(call, tmp_path, case, pick=None, **kw):
    bam_fn, ref_fn = files(tmp_path, case)
    pick = list(range(len(case['sites']))) if pick is None else pick
    out = io.BytesIO()
    call.call_variants(bam_fn, ref_fn, cc.CTG, [case['sites'][i] for i in pick], dev(case['x'][pick], np.int32), dev(case['probs'][pick], np.float32),
                       [case['refs'][i] for i in pick], out, **kw)
    return out.getvalue().decode().splitlines()


@pytest.mark.parametrize('seed,all_bases,haploid,show,qual', [(11, True, False, True, 100), (12, False, False, False, None), (13, True, True, True, 300),
                                                              (14, False, False, True, None)])
def test_lines_equal_the_restatement(call, tmp_path, seed, all_bases, haploid, show, qual):
    """both modes of the indel bases, haploid, showRef, qual; ties between classes and within a list (eighths), all-zero rows"""
    case = cc.cached_case(seed, long_events=seed > 12)
    want = [w[0] for w in cc.expected_rows(case, all_bases, haploid, show, qual) if w is not None]
    got = lines_of(call, tmp_path, case, pysam_for_all_indel_bases=all_bases, haploid=haploid, show_reference=show, qual=qual)
    assert got == want and len(want) > 40


def test_an_insertion_directly_followed_by_a_deletion(call, tmp_path, capsys):
    """the first tensor's line is the restatement's, with `-2NN` in the ALT; the second, whose key passes 50 bytes, is left out"""
    case = cc.insdel_case()
    got = lines_of(call, tmp_path, case, pysam_for_all_indel_bases=True)
    want = cc.expected_rows(dict(case, sites=case['sites'][:1]), True)[0][0]
    assert got == [want] and '-2NN\t' in want and 'left out' in capsys.readouterr().err


CLASSES = set()


@pytest.mark.parametrize('seed,all_bases', [(11, True), (12, False), (13, True), (14, False)])
def test_rows_are_bit_exact_and_every_class_is_there(call, tmp_path, seed, all_bases):
    case = cc.cached_case(seed, long_events=seed > 12)
    bam_fn, ref_fn = files(tmp_path, case)
    events = call.indel_events(bam_fn, cc.CTG, case['sites'], len(case['seq']))
    rows, alleles, status = call.decode(case['sites'], dev(case['x'], np.int32), dev(case['probs'], np.float32), case['refs'], events, case['seq'].encode(),
                                        pysam_for_all_indel_bases=all_bases, show_reference=True)
    want = cc.expected_rows(case, all_bases, False, True)
    assert [i for i, s in enumerate(status) if s == 0] == [i for i, w in enumerate(want) if w is not None] == rows['site'].tolist()
    for row, w in zip(rows, [w for w in want if w is not None]):
        p = w[1]
        assert row['p'].tobytes() == np.float32(p['p']).tobytes() and row['supported'] == p['support'] and row['depth'] == p['depth']
        assert row['flags'] == sum(1 << i for i, f in enumerate(p['flags']) if f) and row['gt21'] == p['gt21'] and row['genotype_task'] == p['task']
        CLASSES.add(int(row['flags'] & -row['flags']).bit_length() - 1)
    assert seed != 14 or CLASSES == set(range(10)), CLASSES          # (the last case: the device emitted each of the ten classes)


def test_the_two_deletion_reset(call, tmp_path):
    case = cc.reset_case()
    got = lines_of(call, tmp_path, case, pysam_for_all_indel_bases=True, show_reference=True)
    assert got == [w[0] for w in cc.expected_rows(case, True, False, True)] and len(got) == 1


def test_alone_in_a_batch_of_257_and_twice(call, tmp_path):
    a, b, c = cc.cached_case(11), cc.cached_case(12), cc.cached_case(14, long_events=True)
    assert a['lines'] != b['lines']
    case = cc.cached_case(11)
    pick = [i % len(case['sites']) for i in range(257)]                   # 257 tensors: positions repeat, as deep sites do
    many = lines_of(call, tmp_path, case, pick, pysam_for_all_indel_bases=True, show_reference=True)
    again = lines_of(call, tmp_path, case, pick, pysam_for_all_indel_bases=True, show_reference=True)
    assert many == again
    want = cc.expected_rows(case, True, False, True)
    assert many == [want[i][0] for i in pick if want[i] is not None]
    for i in (0, 7, 119):
        alone = lines_of(call, tmp_path, case, [i], pysam_for_all_indel_bases=True, show_reference=True)
        assert alone == ([want[i][0]] if want[i] is not None else [])
    assert lines_of(call, tmp_path, case, [], show_reference=True) == []


def test_quantize_on_the_device(call):
    import torch
    q = np.concatenate([np.arange(0, 1000001, 997), [1000000]])
    texts = np.array(['%d.%06d' % (v // 1000000, v % 1000000) for v in q])
    parsed = texts.astype(np.float32)
    rng = np.random.default_rng(2)
    p = np.concatenate([parsed, rng.random(5000, dtype=np.float32), np.float32([0, 1, 0.5e-6, 1.5e-6, 2.5e-6])])
    got = call.quantize(torch.from_numpy(p.copy()).cuda()).cpu().numpy()
    assert got.tobytes() == ref.quantize(p).tobytes() and got[:len(parsed)].tobytes() == parsed.tobytes()


def test_text_pipeline_equals_the_resident_path(call, tmp_path):
    """mpn-call-vcf --input_probabilities on the lines of --output_for_ensemble equals call_variants with quantize_probs"""
    case = cc.cached_case(12)
    bam_fn, ref_fn = files(tmp_path, case)
    text = ''.join('\t'.join([cc.CTG, str(s), r] + [str(v) for v in x.reshape(-1).tolist()] + ['%.6f' % v for v in p.tolist()]) + '\n'
                   for s, r, x, p in zip(case['sites'], case['refs'], case['x'], case['probs']))
    p = subprocess.run([sys.executable, TOOL, '--input_probabilities', '--bam_fn', bam_fn, '--ref_fn', ref_fn, '--pysam_for_all_indel_bases', '--qual', '50',
                        '--sampleName', 'S1'], input=text.encode(), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    got = p.stdout.decode().splitlines()
    head = [l for l in got if l.startswith('#')]
    assert head[0] == '##fileformat=VCFv4.1' and f'##contig=<ID={cc.CTG},length={len(case["seq"])}>' in head and head[-1].endswith('FORMAT\tS1')
    resident = lines_of(call, tmp_path, case, pysam_for_all_indel_bases=True, qual=50, quantize_probs=True)
    assert [l for l in got if not l.startswith('#')] == resident and len(resident) > 20
    quantized = dict(case, probs=ref.quantize(case['probs']))
    assert resident == [w[0] for w in cc.expected_rows(quantized, True, False, False, 50) if w is not None]


def test_refusals(call, tmp_path, capsys):
    import torch
    case = cc.cached_case(11)
    bam_fn, ref_fn = files(tmp_path, case)
    events = call.indel_events(bam_fn, cc.CTG, case['sites'], len(case['seq']))
    x, p = dev(case['x'], np.int32), dev(case['probs'], np.float32)
    for wrong_x, wrong_p in ((x.to(torch.int64), p), (x, p.to(torch.float64)), (x[:, :, :, :2], p), (x, p[:, :80]), (x.cpu(), p), (x[:5], p)):
        with pytest.raises(ValueError):
            call.decode(case['sites'], wrong_x, wrong_p, case['refs'], events, case['seq'].encode())
    with pytest.raises(ValueError, match='not among the sites'):
        call.decode([s + 1000 for s in case['sites']], x, p, case['refs'], events, case['seq'].encode())
    nan = p.clone()
    nan[3, 5] = float('nan')
    with pytest.raises(ValueError, match='NaN'):
        call.decode(case['sites'], x, nan, case['refs'], events, case['seq'].encode())
    assert call.main(['--debug', '--bam_fn', bam_fn, '--ref_fn', ref_fn]) == 2
    assert call.main(['--output_for_ensemble', '--bam_fn', bam_fn, '--ref_fn', ref_fn]) == 2
    assert 'bin/mpn-call-var' in capsys.readouterr().err


def test_the_four_tools_compose_to_the_resident_path(call, tmp_path):
    """mpn-candidates | mpn-create-tensor | mpn-call-var --output_for_ensemble | mpn-call-vcf --input_probabilities with constructed
    weights equals call_variants on the resident blocks with quantize_probs; mpn-call-vcf --chkpnt_fn on the tensor lines equals
    call_variants on the raw probabilities"""
    import clair_net_ref
    from megapath_nano_amd import clair_net, clair_tensor
    from test_clair_checkpoint import write_bundle
    case = cc.decode_case(31, n_sites=1, reads=60, seq=cc.contig(n=700))          # fewer than 100 reads: no draw decides a tensor
    bam_fn, ref_fn = files(tmp_path, case)
    weights = clair_net_ref.seeded_weights(7)
    prefix = os.path.join(str(tmp_path), 'model-000001')
    write_bundle(prefix, weights)
    common = ['--bam_fn', bam_fn, '--ref_fn', ref_fn]

    def tool(name, args, stdin):
        p = subprocess.run([sys.executable, os.path.join(ROOT, 'bin', name)] + args, input=stdin, capture_output=True, timeout=300)
        assert p.returncode == 0, (name, p.stderr.decode()[-2000:])
        return p.stdout
    cand = tool('mpn-candidates', common + ['--ctgName', cc.CTG], b'')
    tens = tool('mpn-create-tensor', common + ['--ctgName', cc.CTG], cand)
    lines = tool('mpn-call-var', ['--chkpnt_fn', prefix, '--tensor_fn', 'PIPE', '--output_for_ensemble'], tens)
    kw = dict(pysam_for_all_indel_bases=True, show_reference=True, qual=100)
    flags = ['--pysam_for_all_indel_bases', '--showRef', '--qual', '100']
    vcf = tool('mpn-call-vcf', common + ['--input_probabilities'] + flags, lines).decode().splitlines()
    direct = tool('mpn-call-vcf', common + ['--chkpnt_fn', prefix, '--tensor_fn', 'PIPE'] + flags, tens).decode().splitlines()
    positions = np.array([int(l.split()[1]) for l in cand.decode().splitlines()])
    assert len(positions) > 10
    centres, block, strings = clair_tensor.tensors(bam_fn, ref_fn, positions, cc.CTG, rng=random.Random(0))
    net = clair_net.ClairNet(weights)
    probs = net.predict(block)
    for quantized, got in ((True, vcf), (False, direct)):
        out = io.BytesIO()
        call.call_variants(bam_fn, ref_fn, cc.CTG, centres, block, probs, strings, out, quantize_probs=quantized, **kw)
        want = out.getvalue().decode().splitlines()
        assert [l for l in got if not l.startswith('#')] == want and len(want) > 10
        assert got[0] == '##fileformat=VCFv4.1'
    net.close()


@pytest.mark.parametrize('name', cc.GOLDEN_NAMES)
def test_every_golden_row(call, tmp_path, name):
    """mpn-call-vcf --input_probabilities on the lines the reference's own call_var.py was given: its header and every record but
    for QUAL, GQ and AF (float32 under the NumPy 2 the fixture was recorded with), and those as the restatement in 'legacy' has them"""
    case = cc.golden_case(name)
    bam_fn, ref_fn = files(tmp_path, case)
    p = subprocess.run([sys.executable, TOOL, '--input_probabilities', '--bam_fn', bam_fn, '--ref_fn', ref_fn] + case['options'],
                       input=case['input'].encode(), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    got, want = p.stdout.decode(), case['vcf']
    assert [l for l in got.splitlines() if l.startswith('#')] == [l for l in want.splitlines() if l.startswith('#')]
    assert [cc.without_float64_columns(l) for l in cc.records(got)] == [cc.without_float64_columns(l) for l in cc.records(want)]
    assert cc.records(got) == [w[0] for w in cc.expected_rows(case, **case['kw']) if w is not None]
