"""GPU test (-m gpu) of the chain of bin/runClair-ensemble.sh for one contig (clair_ensemble.call_ensemble): a tiny sorted BAM with
two sites under 250 reads (three tensors each) and some under fewer than 100, two networks with seeded random weights.  One record
per position where the raw block gives three; the unfiltered VCF is the restatement's decoding (tests/clair_call_ref.py) of the host
build's ensemble of the downloaded probabilities; the filtered one is the restatement's filter of it."""
import collections
import gzip
import io
import os
import random

import numpy as np
import pytest

import clair_call_cases as cc
import clair_ensemble_cases as ec
import clair_ensemble_ref as eref
import pileup_cases as pc

pytestmark = pytest.mark.gpu
DEEP = (81, 111)            # 1-based positions under 250 reads


def reads_of(seq):
    """250 reads over [40, 144) with SNPs at 80 and 110 (0-based) in three of five; 40 reads over [220, 302) with a SNP at 250, a
    deletion of 262 .. 264 in seven of ten, a SNP at 263 in the others and an insertion behind 280 in every second"""
    other = {'A': 'C', 'C': 'G', 'G': 'T', 'T': 'A'}
    rows = []
    for i in range(250):
        start = 40 + i % 5
        s = list(seq[start:start + 100])
        if i % 5 < 3:
            for at in (80, 110):
                s[at - start] = other[seq[at]]
        rows.append((start, len(rows), cc.sam('a%d' % i, 16 if i % 2 else 0, start, '100M', ''.join(s))))
    for i in range(40):
        start = 220 + i % 3
        s = list(seq[start:start + 80])
        s[250 - start] = other[seq[250]]
        if i % 10 < 7:
            cigar, s = '%dM3D%dM' % (262 - start, start + 80 - 265), s[:262 - start] + s[265 - start:]
        else:
            s[263 - start] = other[seq[263]]
            cigar = '80M'
        if i % 2 and cigar == '80M':
            cigar, s = '%dM2I%dM' % (281 - start, start + 80 - 281), s[:281 - start] + ['G', 'G'] + s[281 - start:]
        rows.append((start, len(rows), cc.sam('b%d' % i, 16 if i % 2 else 0, start, cigar, ''.join(s))))
    rows.sort(key=lambda t: t[:2])
    return [t[2] for t in rows]


@pytest.fixture(scope='module')
def chain(libmpn, tmp_path_factory):
    """everything the checks below share: the files, the raw block, both networks' probabilities and what call_ensemble wrote"""
    import clair_net_ref
    from megapath_nano_amd import candidates, clair_call, clair_ensemble, clair_net, clair_tensor
    d = str(tmp_path_factory.mktemp('clair_ensemble_e2e'))
    seq = cc.contig(seed=8, n=400)
    lines = reads_of(seq)
    bam_fn = pc.write_bam(os.path.join(d, 'in.bam'), [(cc.CTG, seq)], lines)
    ref_fn = pc.write_fasta(os.path.join(d, 'ref.fa'), [(cc.CTG, seq)])
    nets = [clair_net.ClairNet(clair_net_ref.seeded_weights(s)) for s in (7, 8)]
    timings = {}
    counts = clair_ensemble.call_ensemble(bam_fn, ref_fn, None, None, os.path.join(d, 'out'), nets=nets, rng=random.Random(0), show_reference=True, timings=timings)
    positions = clair_ensemble.candidate_positions(bam_fn, candidates.read_contig(ref_fn, cc.CTG), cc.CTG)
    centres, block, refs = clair_tensor.tensors(bam_fn, ref_fn, positions, cc.CTG, rng=random.Random(0))
    probs = [net.predict(block) for net in nets]
    raw = io.BytesIO()
    clair_call.call_variants(bam_fn, ref_fn, cc.CTG, centres, block, probs[0], refs, raw, show_reference=True, pysam_for_all_indel_bases=True)
    for net in nets:
        net.close()
    return dict(d=d, seq=seq, lines=lines, bam_fn=bam_fn, ref_fn=ref_fn, counts=counts, centres=centres, refs=refs, x=block.cpu().numpy(),
                probs=[p.cpu().numpy() for p in probs], raw=raw.getvalue().decode().splitlines(), timings=timings)


def rows_of(path):
    with gzip.open(path, 'rt') as f:
        return f.read()


def test_one_record_per_position_where_the_raw_block_gives_three(chain):
    per_centre = collections.Counter(chain['centres'])
    assert all(per_centre[p] == 3 for p in DEEP) and sum(1 for n in per_centre.values() if n == 1) >= 3 and max(per_centre.values()) == 3
    raw = collections.Counter(int(r.split('\t')[1]) for r in chain['raw'])
    assert all(raw[p] == 3 for p in DEEP)
    text = rows_of(os.path.join(chain['d'], 'out', 'snp_and_indel.vcf.gz'))
    got = collections.Counter(int(r.split('\t')[1]) for r in text.splitlines() if r[0] != '#')
    assert set(got.values()) == {1} and all(p in got for p in DEEP) and set(got) <= set(per_centre)
    assert chain['counts'][0] == len(got) and 'ensemble_device_ms' in chain['timings'] and 'overlap_filter' in chain['timings']


def test_the_unfiltered_vcf_is_the_restatement_on_the_host_builds_ensemble(chain, tmp_path):
    from megapath_nano_amd import clair_call
    exe = ec.build_host_check(tmp_path)
    n, k = len(chain['centres']), 2
    keys = list(chain['centres']) * k
    site_off, site_lines, out_slot, n_out, first = ec.grouping(keys, (k + 2) // 2)
    p, host = ec.run_host(exe, tmp_path, ec.case_bytes([i % n for i in range(k * n)], list(range(k * n)), chain['x'].reshape(n, -1), np.concatenate(chain['probs']),
                                                       site_off, site_lines, out_slot, n_out))
    assert p.returncode == 0 and host[0] == -1 and n_out == len(set(chain['centres']))
    sites = [keys[f] for f in first]
    case = dict(seq=chain['seq'], lines=chain['lines'], sites=sites, x=host[1].reshape(-1, 33, 8, 4), probs=host[2], refs=[chain['refs'][f] for f in first])
    want = [w[0] for w in cc.expected_rows(case, True, False, True) if w is not None]
    want.sort(key=lambda r: int(r.split('\t')[1]))
    text = rows_of(os.path.join(chain['d'], 'out', 'snp_and_indel.vcf.gz'))
    assert text == clair_call.vcf_header('Amplicon', chain['ref_fn']) + ''.join(r + '\n' for r in want) and len(want) >= 5


def test_the_filtered_vcf_and_its_reader(chain):
    from megapath_nano_amd import local_realign
    text = rows_of(os.path.join(chain['d'], 'out', 'snp_and_indel.vcf.gz'))
    path = os.path.join(chain['d'], 'out', 'snp_and_indel.filtered.vcf.gz')
    filtered = rows_of(path)
    assert filtered == eref.overlap_text(text)
    positions = [int(r.split('\t')[1]) for r in filtered.splitlines() if r[0] != '#']
    assert local_realign.vcf_positions(path, cc.CTG) == positions and chain['counts'][1] == len(positions) > 0
    with open(path, 'rb') as f:
        raw = f.read()
    assert raw[:4] == b'\x1f\x8b\x08\x04' and raw[12:14] == b'BC' and not os.path.exists(path + '.tbi')          # BGZF, and no index


def test_several_contigs_want_a_name(libmpn, tmp_path):
    from megapath_nano_amd import clair_ensemble
    seq = cc.contig(seed=8, n=400)
    bam_fn = pc.write_bam(os.path.join(str(tmp_path), 'two.bam'), [(cc.CTG, seq), ('other', seq)], reads_of(seq)[:5])
    ref_fn = pc.write_fasta(os.path.join(str(tmp_path), 'ref.fa'), [(cc.CTG, seq), ('other', seq)])
    with pytest.raises(ValueError, match='2 contigs'):
        clair_ensemble.call_ensemble(bam_fn, ref_fn, [], None, os.path.join(str(tmp_path), 'out'), nets=[])
    with pytest.raises(ValueError, match='one contig per call'):
        clair_ensemble.call_ensemble(bam_fn, ref_fn, [], [cc.CTG, 'other'], os.path.join(str(tmp_path), 'out'), nets=[])
