"""CPU test: the restatement of realign_illumina_reads.py (tests/read_realign_ref.py) reproduces, byte for byte, every record that the
reference's unmodified script printed for the golden cases (tests/golden/read_realign/, recorded by
tests/golden/make_read_realign_golden.py with the project's own graph consensus behind the script's binding), with the project's
plain restatements of the consensus (tests/dbg_ref.py) and of the realigner (oracle/realign_oracle.py) as its two libraries."""
import os

import pytest

import read_realign_cases as rc
import read_realign_ref as ref

GOLDEN, load = rc.GOLDEN, rc.load_golden


def test_the_goldens_reach_what_they_are_for():
    golds = [load(p)[0] for p in GOLDEN]
    assert len(golds) >= 10 and sum(g['changed'] > 0 for g in golds) >= 3


@pytest.mark.parametrize('path', GOLDEN, ids=[os.path.basename(p)[:-8] for p in GOLDEN])
def test_restatement_reproduces_the_script(path, oracle_built):
    gold, case = load(path)
    trace = []
    lines = ref.realign(rc.sam_lines(case), case['contig'], rc.CTG, case['min_mq'], case['min_coverage'], trace=trace)
    assert lines == gold['records']
    assert ''.join(gold['header']) == rc.header_text(case)
    names = [l.split('\t')[0] for l in lines]
    assert len(set(names)) == len(names) and all(l.endswith('\n') and len(l.split('\t')) == 12 for l in lines)


def test_the_products_host_rules_equal_the_restatements():
    """the names, the windows of a row and the fold of realignment results: the product's closed forms against the serial ones"""
    import random
    from megapath_nano_amd import read_realign as rr
    assert rr.CHAR_STR == ref.ALPHABET and len(rr.CHAR_STR) == 87
    for i in (0, 1, 86, 87, 87 ** 2 + 5, 87 ** 5 - 1, 87 ** 5, 87 ** 5 + 88):
        assert rr.read_name(i) == ref.name_of(i)
    assert [rr.read_name(i) for i in (0, 86, 87, 87 ** 5 - 1, 87 ** 5)] == ['00000', '0000~', '00010', '~~~~~', '00000']
    rng = random.Random(3)
    for _ in range(50):
        start = rng.randrange(0, 20000)
        cand = sorted(set(rng.randrange(start - 21, start + 5020) for _ in range(rng.randrange(1, 40))))
        want = [ref.windows_of([p for p in cand if start + 1000 * s - 21 <= p < start + 1000 * s + 1020]) for s in range(5)]
        assert rr.chunk_windows(cand, start) == want
    assert rr.chunk_windows([100, 260, 421], 0)[0] == [(20, 340), (341, 501)]
    for _ in range(200):
        read, rec = rr.Read(), dict(pos=100, cigar='50M', best=(100, '50M', None))
        read.pos, read.cigar, read.best_pos, read.best_cigar, read.best_score = 100, '50M', 100, '50M', None
        for _ in range(4):
            position, cigar = rng.choice((100, 101)), rng.choice(('50X', '50M', '20X2D30X', '20X1I29X', '10S40X', '25X2D25X'))
            read.realigned(position, cigar)
            ref.accept(rec, position, cigar)
            assert (read.best_pos, read.best_cigar, read.best_score) == rec['best']
