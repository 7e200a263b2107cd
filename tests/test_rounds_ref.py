"""The iterated consensus without a GPU: the oracle of tests/rounds_ref.py (include/pw_rounds.h restated) against
tests/polish_ref.py on the planted pileup, the three branches of the remap, and the rounds on the noisy fixture of
tests/consensus_cases.py on the oracle side, pinned to the figures the rounds were proposed with:

    stage     errors against the genome   contig length   record (kept, substituted, deleted, inserted)
    draft     136
    round 1    14                          1987            (1892, 72, 32, 23)
    round 2    11                          1990            (1987, 0, 0, 3)
    round 3    10                          1991            (1990, 0, 0, 1)
    round 4    10                          1991            (1991, 0, 0, 0)

125 tasks and 125 aligned in every round; round 4 is a fixed point."""
import numpy as np
import pytest

from tests import consensus_cases as CC
from tests import polish_plant_cases as PP
from tests import polish_ref as PR
from tests import rounds_cases as RC
from tests import rounds_ref as RR

TABLE = [(14, 1987, (1892, 72, 32, 23)), (11, 1990, (1987, 0, 0, 3)), (10, 1991, (1990, 0, 0, 1)), (10, 1991, (1991, 0, 0, 0))]


@pytest.mark.parametrize('min_depth', (3, 2))
def test_column_polish_equals_the_per_read_polish(min_depth):
    counts, ins, frame = PP.counts(), PP.expected_plane(), PP.frame()
    for offs, lens in RC.ordered_read_sets():
        want, wstats = PR.polish(counts, ins, PP.L, frame, offs, lens, min_depth)
        got, stats, colmap = RR.column_polish(counts, ins, PP.L, frame, offs, lens, min_depth)
        assert got == want and stats.tolist() == wstats.tolist()
        assert len(colmap) == PP.N_COLS + 1 and colmap[0] == 0 and (np.diff(colmap.astype(np.int64)) >= 0).all()
        assert int(colmap[-1]) == sum(len(r) for r in want)
        for r, (off, n) in enumerate(zip(offs, lens)):
            assert int(colmap[off + n]) - int(colmap[off]) == len(want[r])
    sets = RC.ordered_read_sets()
    assert any(0 in lens for _, lens in sets) and max(len(o) for o, _ in sets) == 1000
    for bad in (([0, 5], [6, 3]), ([10, 0], [3, 3]), ([298], [3]), ([-1], [1])):
        with pytest.raises(ValueError):
            RR.column_polish(counts, ins, PP.L, frame, *bad)


def test_remap_branches_and_monotony():
    rng = np.random.default_rng(7820)
    n = 40
    e = rng.integers(0, 4, n)
    emap = np.concatenate([[0], np.cumsum(e)])
    got = [RR.remap(p, n, emap) for p in range(-8, n + 9)]
    assert all(a <= b for a, b in zip(got, got[1:]))
    assert [RR.remap(p, n, emap) for p in (-5, 0, n, n + 5)] == [-5, 0, int(emap[n]), int(emap[n]) + 5]
    ident = np.arange(n + 1)
    assert [RR.remap(p, n, ident) for p in range(-8, n + 9)] == list(range(-8, n + 9))
    assert RR.remap(3, 0, [0]) == 3 and RR.remap(0, 0, [0]) == 0            # a contig of no letters


def test_rounds_on_the_noisy_fixture_reproduce_the_table(oracle):
    nf = CC.noisy_fixture()
    fx, genome = nf['fx'], nf['genome']
    draft, rounds = RR.oracle_rounds(oracle, fx['reads'], CC.oracle_records(oracle), 5)
    errors = [CC.errors(r['contigs'], genome) for r in rounds]
    print('draft %d; rounds: %r' % (CC.errors(draft, genome),
                                    [(e, [len(c) for c in r['contigs']], r['stats'].tolist(), len(r['tasks']), r['aligned'])
                                     for e, r in zip(errors, rounds)]))
    assert CC.errors(draft, genome) == 136
    assert len(rounds) == 4                                                  # round 4 is the fixed point: the loop stops there
    for (err, length, rec), e, r in zip(TABLE, errors, rounds):
        assert e == err and [len(c) for c in r['contigs']] == [length] and r['stats'].tolist() == [rec]
        assert len(r['tasks']) == 125 and r['aligned'] == 125
    assert errors[1] <= errors[0] and errors[2] <= errors[1]
    assert (rounds[3]['contigs'][0] == rounds[2]['contigs'][0]).all()
    # one round of the rounds is the single-round consensus
    single = CC.oracle_consensus(oracle, fx['reads'], CC.oracle_records(oracle))
    assert (single['contigs'][0] == rounds[0]['contigs'][0]).all() and single['stats'].tolist() == rounds[0]['stats'].tolist()
    assert RR.oracle_rounds(oracle, fx['reads'], CC.oracle_records(oracle), 1)[1][0]['stats'].tolist() == rounds[0]['stats'].tolist()


def test_exports_match_the_header():
    import os
    import re
    from biseqt_amd import _pwlib as W
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, 'include', 'pw_rounds.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    declared = set(re.findall(r'\b(pw_\w+)\s*\(', txt))
    assert declared == set(W.ROUNDS_EXPORTS), declared ^ set(W.ROUNDS_EXPORTS)
    lib = W.load()
    for name in declared:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name


def test_the_wide_fixture_holds_what_it_is_for(oracle):
    """The plane the planted pairs give (by CPU-oracle GLOBAL alignments) has a column that emits nine letters, columns whose
    slots pass and fail, and the read sets have reads of 255, 256 and 257 columns, gaps of 0, 1 and 3, an unread head and tail,
    and a last read that ends at n_cols."""
    counts0, ins = PR.zeros(RC.WIDE_COLS, RC.WIDE_L, RC.WIDE_J)
    for o, m in RC.wide_pairs():
        res = oracle.solve(o, m, mode=oracle.STD_MODE, alntype=oracle.GLOBAL, L=RC.WIDE_L, match=PP.GAPPY['match_score'],
                           mismatch=PP.GAPPY['mismatch_score'], go=PP.GAPPY['go_score'], ge=PP.GAPPY['ge_score'])
        PR.add(counts0, ins, RC.WIDE_L, 0, len(o), res['origin_idx'], res['mutant_idx'], res['transcript'], m)
    counts, nine = RC.wide_counts(ins)
    assert len(nine) >= 1 and ins[:, 7].any()
    frame = RC.wide_frame()
    for offs, lens in RC.WIDE_READ_SETS:
        want, wstats = PR.polish(counts, ins, RC.WIDE_L, frame, offs, lens, 1)
        got, stats, colmap = RR.column_polish(counts, ins, RC.WIDE_L, frame, offs, lens, 1)
        assert got == want and stats.tolist() == wstats.tolist()
    e = np.diff(RR.column_polish(counts, ins, RC.WIDE_L, frame, [0], [RC.WIDE_COLS], 1)[2].astype(np.int64))
    assert e.max() == 9 and e.min() == 0 and {1, 2, 3} <= set(e.tolist())
    (offs, lens), (offs2, lens2) = RC.WIDE_READ_SETS[:2]
    assert lens[:3] == [255, 256, 257] and [offs[k + 1] - offs[k] - lens[k] for k in range(3)] == [0, 1, 3]
    assert offs[0] > 0 and offs[-1] + lens[-1] < RC.WIDE_COLS and offs2[-1] + lens2[-1] == RC.WIDE_COLS
