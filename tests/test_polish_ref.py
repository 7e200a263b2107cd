"""Read correction without a GPU: the oracle of tests/polish_ref.py on hand-written transcripts with hand-written expected
arrays, its origin-side counts against tests/pileup_ref.py, and the correction experiment on synthetic reads of both strands
with the CPU oracle's alignments.

The experiment as run here (tests/polish_cases.py: a 1500-letter genome, 45 reads of 400 letters, 3 % substitutions, 2 %
insertions, 2 % deletions, 398 true overlaps of at least 150 letters, B_OVERLAP 1 / -3 / -5 / -2 in a band of +-40): total
edit distance to the truth 1211 uncorrected, 196 corrected (two slots, min_depth 3), 391 without insertion slots."""
import numpy as np

from tests import pileup_ref as R
from tests import polish_cases as PC
from tests import polish_ref as PR

L, DEL, INS = 4, 4, 5


def _expect(n_cols, J, cells, slots):
    counts, ins = PR.zeros(n_cols, L, J)
    for (col, ch), v in cells.items():
        counts[col, ch] = v
    for (col, j, y), v in slots.items():
        ins[col, j, y] = v
    return counts, ins


def _same(got, want):
    return (got[0] == want[0]).all() and (got[1] == want[1]).all()


def test_leading_trailing_and_long_insertion_runs():
    """'IMIIIMI' at frame start 1, origin_idx 1 (c = 2), two slots: the leading I is anchored nowhere, the run of three gives
    ONE event and its first two letters, the trailing I is anchored to the last column."""
    got = PR.zeros(6, L, 2)
    PR.add(*got, L, 1, 4, 1, 0, 'IMIIIMI', [3, 0, 1, 2, 3, 1, 2])
    want = _expect(6, 2, {(2, 0): 1, (2, INS): 1, (3, 1): 1, (3, INS): 1}, {(2, 0, 1): 1, (2, 1, 2): 1, (3, 0, 2): 1})
    assert _same(got, want), got
    PR.add(*got, L, 1, 4, 1, 0, 'IMIIIMI', [3, 0, 1, 2, 3, 1, 2])                    # cumulative
    assert _same(got, (2 * want[0], 2 * want[1]))
    one = PR.zeros(6, L, 1)                                                         # one slot: the first letter only
    PR.add(*one, L, 1, 4, 1, 0, 'IMIIIMI', [3, 0, 1, 2, 3, 1, 2])
    assert _same(one, _expect(6, 1, {(2, 0): 1, (2, INS): 1, (3, 1): 1, (3, INS): 1}, {(2, 0, 1): 1, (3, 0, 2): 1}))
    none = PR.zeros(6, L, 0)                                                        # no plane: the counts alone
    PR.add(*none, L, 1, 4, 1, 0, 'IMIIIMI', [3, 0, 1, 2, 3, 1, 2])
    assert none[1] is None and (none[0] == want[0]).all()


def test_i_directly_followed_by_d_and_a_letter_outside_the_alphabet():
    got = PR.zeros(3, L, 2)
    PR.add(*got, L, 0, 3, 0, 1, 'MIDM', [0, 1, 2, 3])                               # mutant_idx 1: the letters read are 1, 2, 3
    assert _same(got, _expect(3, 2, {(0, 1): 1, (0, INS): 1, (1, DEL): 1, (2, 3): 1}, {(0, 0, 2): 1})), got
    got = PR.zeros(2, L, 2)
    PR.add(*got, L, 0, 1, 0, 0, 'MII', [0, 9, 2])                                    # slot 0 holds a letter >= L: nothing there
    assert _same(got, _expect(2, 2, {(0, 0): 1, (0, INS): 1}, {(0, 1, 2): 1})), got
    got = PR.zeros(3, L, 2)
    PR.add(*got, L, 0, 3, 0, 0, 'MIDIM', [1, 2, 3, 0])                               # a D between two I: two runs, two events
    assert _same(got, _expect(3, 2, {(0, 1): 1, (0, INS): 1, (1, DEL): 1, (1, INS): 1, (2, 0): 1}, {(0, 0, 2): 1, (1, 0, 3): 1})), got


def test_a_leading_d_seen_from_the_mutant_side_is_anchored_nowhere():
    assert PR.swap('DMIS') == 'IMDS'
    got = PR.zeros(4, L, 2)
    PR.add_mutant_side(*got, L, 1, [1, 2, 3], 2, 0, 0, 'DMM')                        # swapped: 'IMM' over the origin's letters
    assert _same(got, _expect(4, 2, {(1, 2): 1, (2, 3): 1}, {})), got
    got = PR.zeros(4, L, 2)
    PR.add_mutant_side(*got, L, 1, [1, 2, 3], 2, 0, 0, 'MDM')                        # an inner D: the deleted letter is recorded
    assert _same(got, _expect(4, 2, {(1, 1): 1, (1, INS): 1, (2, 3): 1}, {(1, 0, 2): 1})), got
    got = PR.zeros(4, L, 2)
    PR.add_mutant_side(*got, L, 3, [1, 2, 3], 2, 0, 0, 'MDM')                        # the mutant frame overhangs by one column
    assert not got[0].any() and not got[1].any()


def test_a_reversed_pair_worked_out_by_hand():
    """Read b = 0 1 1 2 3; the mutant frame is rc(b) = 0 1 2 2 3 under the complement 3 2 1 0.  The origin frame 1 2 0 3 3
    aligns from origin_idx 1, mutant_idx 1 with 'IMDSM' (o(n) = m(n) = 4).  By the definition: reverse(swap(t)) = 'MSIMD',
    origin_idx' = 5 - (1 + 4) = 0, mutant_idx' = 5 - (1 + 4) = 0, rc(origin frame) = 0 0 3 1 2.  So b[0] sees a 0, b[1] a 0 and,
    behind it, the inserted 3 (the complement of the deleted origin letter 0), b[2] a 1, b[3] is deleted, b[4] is not covered."""
    got = PR.zeros(8, L, 2)
    PR.add_mutant_side_reversed(*got, L, 2, [1, 2, 0, 3, 3], 5, 1, 1, 'IMDSM', [3, 2, 1, 0])
    want = _expect(8, 2, {(2, 0): 1, (3, 0): 1, (3, INS): 1, (4, 1): 1, (5, DEL): 1}, {(3, 0, 3): 1})
    assert _same(got, want), got
    # the same thing said the long way: rc(b) against the origin IS b against rc(origin), read from the other end
    direct = PR.zeros(8, L, 2)
    PR.add(*direct, L, 2, 5, 0, 0, 'MSIMD', [0, 0, 3, 1, 2])
    assert _same(got, direct)


def test_origin_side_counts_equal_the_pileup_oracle():
    rng = np.random.default_rng(7600)
    for _ in range(200):
        n = int(rng.integers(1, 40))
        tx = ''.join(rng.choice(list('MMMSID'), n))
        X = sum(tx.count(c) for c in 'MSD') + int(rng.integers(0, 3))
        oi, mi = int(rng.integers(0, 3)), int(rng.integers(0, 3))
        mutant = rng.integers(0, 6, mi + n + 1)                                     # letters 4 and 5 lie outside the alphabet
        f = int(rng.integers(0, 4))
        n_cols = f + X + oi + int(rng.integers(0, 2))
        want = R.zeros(n_cols, L)
        R.add(want, L, f, X + oi, oi, mi, tx, mutant)
        for J in (0, 1, 3):
            got = PR.zeros(n_cols, L, J)
            PR.add(*got, L, f, X + oi, oi, mi, tx, mutant)
            assert (got[0] == want).all(), tx
            if J:                                                                   # slot 0: at most one letter per anchored event
                assert (got[1][:, 0].sum(axis=1) <= want[:, INS]).all()


def test_polish_rule_by_hand():
    """One read of five columns over L = 2, J = 2: a tie between the letters (the lower), DEL wins, below min_depth (the
    read's own letter), an insertion whose first slot passes and whose second fails, a tie of a letter with DEL (the letter)."""
    counts = np.array([[2, 2, 0, 0], [1, 0, 2, 0], [1, 0, 0, 0], [0, 3, 0, 2], [1, 0, 1, 0]], np.uint32)
    ins = np.zeros((5, 2, 2), np.uint32)
    ins[3, 0] = (1, 1)                                        # n_0 = 2, 2 * 2 > 3: emitted, a tie: letter 0
    ins[3, 1] = (0, 1)                                        # n_1 = 1, 2 * 1 > 3 fails
    ins[2, 0] = (5, 0)                                        # below min_depth: nothing is inserted
    reads, stats = PR.polish(counts, ins, 2, [1, 1, 1, 1, 1], [0], [5], min_depth=2)
    assert reads == [[0, 1, 1, 0, 0]]
    assert stats.tolist() == [(2, 2, 1, 1)]                   # kept: columns 2 and 3; substituted: 0 and 4; deleted: 1; inserted: 1
    reads, stats = PR.polish(counts, None, 2, [1, 1, 1, 1, 1], [0, 5, 1], [5, 0, 2], min_depth=1)
    assert reads == [[0, 0, 1, 0], [], [0]] and stats.tolist() == [(1, 3, 1, 0), (0, 0, 0, 0), (0, 1, 1, 0)]


def test_edit_distance():
    assert PR.edit_distance([0, 1, 2, 3], [0, 1, 2, 3]) == 0 and PR.edit_distance([], [1, 2]) == 2
    assert PR.edit_distance([0, 1, 2, 3], [0, 2, 2, 3, 3]) == 2 and PR.edit_distance([0, 1, 2], []) == 3
    assert PR.edit_distance([0, 0, 0, 1], [1, 0, 0, 0]) == 2


def test_correction_experiment_with_the_cpu_oracle(oracle):
    """Both strands, known positions, the oracle's alignments, both sides piled: the corrected reads' total edit distance to
    the truth is less than half of the uncorrected reads' -- a floor that a rule that does nothing misses, not the expected
    value (the module docstring has the figures)."""
    from biseqt_amd.batch import pack_reads
    fx = PC.fixture()
    alns = PC.oracle_alignments(oracle, fx)
    assert '-' in fx['strands'] and '+' in fx['strands'] and sum(a is not None for a in alns) >= 300
    arena, offs, lens = pack_reads(fx['reads'])
    counts, ins = PC.pileup_of(fx['reads'], offs, arena.nbytes, fx['pairs'], fx['strands'], alns, PC.INS_SLOTS, PC.SELF_WEIGHT)
    reads, stats = PR.polish(counts, ins, PC.L, arena, offs, lens, PC.MIN_DEPTH)
    before, after = PC.total_distance(fx['reads'], fx['truth']), PC.total_distance(reads, fx['truth'])
    print('total edit distance: uncorrected %d, corrected %d' % (before, after))
    assert 2 * after < before, (before, after)
    assert int(stats['inserted'].sum()) > 0 and int(stats['deleted'].sum()) > 0 and int(stats['substituted'].sum()) > 0
    # the inserted letters are needed: without the slots the same pileup corrects visibly less
    flat, _ = PR.polish(counts, None, PC.L, arena, offs, lens, PC.MIN_DEPTH)
    assert PC.total_distance(flat, fx['truth']) > after
