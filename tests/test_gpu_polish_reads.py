"""The self vote, the polish and the read-correction flows (``Pileup.add_letters`` / ``polish``, ``overlap_alignments(
pileup_sides='both')``, ``polish_reads``, ``correct_reads``; include/pw_polish.h) against the oracle of tests/polish_ref.py:
every comparison is ``==``.

The correction experiment on the device (tests/polish_cases.py, the fixture of tests/test_polish_ref.py): total edit distance
to the truth 1211 uncorrected, 196 corrected -- the same reads as the CPU oracle gives, letter for letter."""
import numpy as np
import pytest

from tests import polish_cases as PC
from tests import polish_plant_cases as PP
from tests import polish_ref as PR

pytestmark = pytest.mark.gpu


def test_add_letters_weights_and_sub_ranges():
    from biseqt_amd.batch import DeviceArena, Pileup
    rng = np.random.default_rng(7810)
    letters = rng.integers(0, 6, 100).astype(np.uint8)                    # 4 and 5 lie outside the alphabet
    host = np.concatenate([np.full(16, 9, np.uint8), letters, np.full(16, 9, np.uint8)])
    want = PR.zeros(100, 4, 0)[0]
    with Pileup(100, 4) as p, DeviceArena(host) as dev:
        p.add_letters(letters[20:70], weight=3, lo=20)
        PR.add_letters(want, 4, letters[20:70], 20, 3)
        assert (p.counts() == want).all() and want.sum() == 3 * int((letters[20:70] < 4).sum())
        p.add_letters(letters)                                            # weight 1, every column, cumulative
        PR.add_letters(want, 4, letters, 0, 1)
        assert (p.counts() == want).all()
        p.add_letters((dev, 16 + 30), weight=2, lo=30)                    # letters that are on the device already
        PR.add_letters(want, 4, letters[30:], 30, 2)
        assert (p.counts() == want).all()
        p.add_letters(letters[:0], lo=100)                                # nothing
        p.add_letters(letters[:5], weight=0)
        assert (p.counts() == want).all() and not want[:, 4:].any()
        for bad in (dict(lo=51), dict(lo=-1)):
            with pytest.raises(ValueError):
                p.add_letters(letters[:50], **bad)
        with pytest.raises(ValueError):
            p.add_letters((dev, len(host) - 50), lo=49)


@pytest.fixture(scope='module')
def planted():
    """The pileup of tests/polish_plant_cases.py: the plane filled by adds of a six-letter batch, the counts set by hand."""
    from biseqt_amd.batch import BatchAligner, Pileup
    with BatchAligner(PP.pairs(), alnmode=0, alntype=0, alphabet_len=6, **PP.GAPPY) as b, Pileup(PP.N_COLS, PP.L, ins_slots=PP.J) as p:
        res = b.run()
        txs = b.transcripts(res)
        b.pileup_add(p, sides='origin', col0=np.zeros(b.n, np.int64), mutant_col0=np.zeros(b.n, np.int64))
        b.sync()
        want = PR.zeros(PP.N_COLS, PP.L, PP.J)
        for k, (o, m) in enumerate(PP.pairs()):
            PR.add(*want, PP.L, 0, len(o), int(res['origin_idx'][k]), int(res['mutant_idx'][k]), txs[k], m)
        ins = p.ins_counts()
        assert (ins == want[1]).all() and (p.counts() == want[0]).all()
        assert (ins == PP.expected_plane()).all()                         # the construction came out as planted
        p.set_counts(PP.counts())
        assert (p.ins_counts() == ins).all()                              # set_counts leaves the plane alone
        yield p, PP.counts(), ins, PP.frame()


@pytest.mark.parametrize('min_depth', (3, 2))
def test_polish_from_planted_counts(planted, min_depth):
    from biseqt_amd.batch import POLISH_STATS_DTYPE, DeviceArena
    p, counts, ins, frame = planted
    host = np.concatenate([np.full(16, 9, np.uint8), frame, np.full(16, 9, np.uint8)])
    with DeviceArena(host) as dev:
        for q, (offs, lens) in enumerate(PP.read_sets()):
            want, wstats = PR.polish(counts, ins, PP.L, frame, offs, lens, min_depth)
            for ref in ((frame, (dev, 16)) if q < 9 else ((dev, 16),)):
                letters, offsets, stats = p.polish(ref, offs, lens, min_depth=min_depth)
                assert letters.dtype == np.uint8 and offsets.dtype == np.int64 and stats.dtype == POLISH_STATS_DTYPE
                assert offsets.tolist() == np.concatenate([[0], np.cumsum([len(r) for r in want])]).tolist()
                assert letters.tolist() == [y for r in want for y in r]
                assert stats.tolist() == wstats.tolist()
    # the constructed columns say what they were built for (min_depth 3 and 2 differ at column 45 only)
    one = [p.polish(frame, [c], [1], min_depth=min_depth)[0].tolist() for c in (10, 20, 30, 33, 40, 45, 46, 50, 60, 61, 62)]
    assert one == [[2, 0], [0, 2], [2], [2, 1], [0], [0] if min_depth == 3 else [0, 2], [2], [0], [0], [3], [1]]
    assert p.polish(frame, [100], [10], min_depth=min_depth)[0].size == 0                       # every column deleted
    full, _, st = p.polish(frame, [120], [5], min_depth=min_depth)
    assert full.tolist() == [0, 1, 2, 3] * 5 and st.tolist() == [(5, 0, 0, 15)]                  # 1 + J letters per column


def test_polish_without_a_plane_and_the_refusals(planted):
    from biseqt_amd import _pwlib as W
    from biseqt_amd.batch import Pileup
    _, counts, _, frame = planted
    lib = W.load()
    out = np.zeros(64, np.int64)
    with Pileup(PP.N_COLS, PP.L) as p:
        # the polished accessors before a polish
        assert lib.pw_pileup_polished_total(p.handle) == -1 and 'before pw_pileup_polish' in W.last_error()
        for name in ('pw_pileup_polished_offsets', 'pw_pileup_polished_letters', 'pw_pileup_polished_stats'):
            assert getattr(lib, name)(p.handle, out.ctypes.data) == -1 and 'before pw_pileup_polish' in W.last_error()
        assert not lib.pw_pileup_polished_letters_device(p.handle) and not lib.pw_pileup_polished_offsets_device(p.handle)
        # a read outside the pileup, refused by the library itself
        for off, ln in ((298, 3), (-1, 1), (301, 0), (0, -1)):
            o, n = np.array([0, off], np.int64), np.array([5, ln], np.int32)
            assert lib.pw_pileup_polish(p.handle, lib.pw_pileup_counts_device(p.handle), o.ctypes.data, n.ctypes.data, 2, 1, None) == -1
            assert 'read 1 lies outside the pileup' in W.last_error()
        assert lib.pw_pileup_polished_total(p.handle) == -1
        p.set_counts(counts)
        want, wstats = PR.polish(counts, None, PP.L, frame, [0, 100, 7], [300, 10, 0], 3)
        letters, offsets, stats = p.polish(frame, [0, 100, 7], [300, 10, 0], min_depth=3)      # no plane: no insertions
        assert letters.tolist() == want[0] and offsets.tolist() == [0, len(want[0]), len(want[0]), len(want[0])]
        assert stats.tolist() == wstats.tolist() and not stats['inserted'].any()
        assert lib.pw_pileup_polished_total(p.handle) == len(want[0])
        assert lib.pw_pileup_polished_letters_device(p.handle) and lib.pw_pileup_polished_offsets_device(p.handle)
        letters, offsets, stats = p.polish(frame, [], [])                                        # no reads
        assert letters.size == 0 and offsets.tolist() == [0] and stats.size == 0


@pytest.fixture(scope='module')
def device_alignments():
    """The fixture's pairs aligned on the device in several batches, both sides piled up: (alignments, counts, plane)."""
    from biseqt_amd.batch import Pileup, pack_reads
    from biseqt_amd.overlap import overlap_alignments
    from biseqt_amd.sequence import Alphabet
    fx = PC.fixture()
    arena, offs, lens = pack_reads(fx['reads'])
    with Pileup(arena.nbytes, PC.L, ins_slots=PC.INS_SLOTS) as p:
        alns = overlap_alignments(fx['reads'], fx['pairs'], fx['bands'], Alphabet('ACGT'), strands=fx['strands'], complement=PC.COMPLEMENT,
                                  want_transcripts=True, pileup=p, pileup_sides='both', max_cells=3 * 10 ** 6)
        return alns, p.counts(), p.ins_counts()


def test_overlap_alignments_pile_both_sides_over_several_batches(device_alignments):
    from biseqt_amd.batch import pack_reads
    fx = PC.fixture()
    alns, counts, ins = device_alignments
    assert sum(a is not None for a in alns) >= 300 and {a['strand'] for a in alns if a} == {'+', '-'}
    cells = sum((a['diag_range'][1] - a['diag_range'][0] + 1) * 400 for a in alns if a)
    assert cells > 2 * 3 * 10 ** 6                                                               # more than two batches
    arena, offs, lens = pack_reads(fx['reads'])
    want = PC.pileup_of(fx['reads'], offs, arena.nbytes, fx['pairs'], fx['strands'], alns, PC.INS_SLOTS, 0)
    assert (counts == want[0]).all(), np.argwhere(counts != want[0])[:8]
    assert (ins == want[1]).all(), np.argwhere(ins != want[1])[:8]
    assert ins[:, 1].any()
    for r in (0, len(offs) - 1):                                                                 # the last read has columns too
        assert counts[int(offs[r]):int(offs[r]) + int(lens[r])].any()


def test_polish_reads_equals_the_oracle_and_halves_the_errors(device_alignments):
    from biseqt_amd.batch import pack_reads
    from biseqt_amd.overlap import polish_reads
    from biseqt_amd.sequence import Alphabet
    fx = PC.fixture()
    alns, _, _ = device_alignments
    arena, offs, lens = pack_reads(fx['reads'])
    counts, ins = PC.pileup_of(fx['reads'], offs, arena.nbytes, fx['pairs'], fx['strands'], alns, PC.INS_SLOTS, PC.SELF_WEIGHT)
    want, wstats = PR.polish(counts, ins, PC.L, arena, offs, lens, PC.MIN_DEPTH)
    stats = {}
    got = polish_reads(fx['reads'], fx['pairs'], fx['bands'], Alphabet('ACGT'), strands=fx['strands'], complement=PC.COMPLEMENT,
                       min_depth=PC.MIN_DEPTH, ins_slots=PC.INS_SLOTS, self_weight=PC.SELF_WEIGHT, stats=stats, max_cells=3 * 10 ** 6)
    assert len(got) == len(fx['reads']) and all(g.dtype == np.uint8 for g in got)
    assert [g.tolist() for g in got] == want
    assert stats['records'].tolist() == wstats.tolist() and stats['aligned'] == sum(a is not None for a in alns)
    assert all(stats[k] >= 0 for k in ('vote_ms', 'align_ms', 'polish_ms'))
    before, after = PC.total_distance(fx['reads'], fx['truth']), PC.total_distance(got, fx['truth'])
    print('total edit distance: uncorrected %d, corrected %d' % (before, after))
    assert 2 * after < before, (before, after)


def test_correct_reads_from_raw_reads_on_both_strands():
    from biseqt_amd.overlap import correct_reads
    from biseqt_amd.sequence import Alphabet
    fx = PC.fixture()
    stats = {}
    got = correct_reads(fx['reads'], 10, Alphabet('ACGT'), .2, .9, p_min=.7, strands='both', complement=PC.COMPLEMENT, stats=stats)
    assert len(got) == len(fx['reads']) and all(isinstance(g, np.ndarray) and g.dtype == np.uint8 and g.ndim == 1 for g in got)
    assert stats['overlaps']['pairs'] > 0 and len(stats['records']) == len(fx['reads'])
    print('correct_reads: %d pairs found, %d aligned; total edit distance %d -> %d'
          % (stats['overlaps']['pairs'], stats['aligned'], PC.total_distance(fx['reads'], fx['truth']), PC.total_distance(got, fx['truth'])))
