"""The column polish (``Pileup.polish(columns=True)``, ``Pileup.colmap``; include/pw_rounds.h, pw_rounds.hip) against the
oracle of tests/rounds_ref.py AND against the per-read polish (``pw_pileup_polish``) on the same pileup: letters, offsets,
total, statistics and the coordinate map are compared with ``==``.  The planted pileup of tests/polish_plant_cases.py over
its read sets (sorted and clipped: the column polish takes no overlapping reads), a pileup of 1100 columns with eight
insertion slots whose reads straddle the 256-column chunks of the grid, a pileup without a plane, and the refusals."""
import numpy as np
import pytest

from tests import polish_plant_cases as PP
from tests import rounds_cases as RC
from tests import rounds_ref as RR

pytestmark = pytest.mark.gpu


def _check(p, ref, counts, ins, L, frame, offs, lens, min_depth):
    """One read set, by columns and by reads, against the oracle."""
    from biseqt_amd import _pwlib as W
    from biseqt_amd.batch import POLISH_STATS_DTYPE
    want, wstats, wmap = RR.column_polish(counts, ins, L, frame, offs, lens, min_depth)
    flat = [y for r in want for y in r]
    woffs = np.concatenate([[0], np.cumsum([len(r) for r in want])]).astype(np.int64).tolist()
    letters, offsets, stats = p.polish(ref, offs, lens, min_depth=min_depth, columns=True)
    assert letters.dtype == np.uint8 and offsets.dtype == np.int64 and stats.dtype == POLISH_STATS_DTYPE
    assert letters.tolist() == flat and offsets.tolist() == woffs and stats.tolist() == wstats.tolist()
    assert int(p.lib.pw_pileup_polished_total(p.handle)) == len(flat)
    colmap = p.colmap()
    assert colmap.dtype == np.uint64 and colmap.tolist() == wmap.tolist()
    assert p.colmap(3, 7).tolist() == wmap[3:7].tolist() and p.colmap(p.n_cols, p.n_cols + 1).tolist() == [wmap[-1]]
    assert p.lib.pw_pileup_colmap_device(p.handle)
    assert [int(colmap[o]) for o in offs] + [int(colmap[-1])] == woffs          # offsets[r] = colmap[read_offs[r]]
    by_read = p.polish(ref, offs, lens, min_depth=min_depth)                    # the per-read polish on the same pileup
    assert by_read[0].tolist() == flat and by_read[1].tolist() == woffs and by_read[2].tolist() == wstats.tolist()
    assert not p.lib.pw_pileup_colmap_device(p.handle) and 'before pw_pileup_polish_columns' in W.last_error()
    return want, wmap


@pytest.fixture(scope='module')
def planted():
    """The pileup of tests/polish_plant_cases.py: the plane filled by adds of a six-letter batch, the counts set by hand."""
    from biseqt_amd.batch import BatchAligner, Pileup
    with BatchAligner(PP.pairs(), alnmode=0, alntype=0, alphabet_len=6, **PP.GAPPY) as b, Pileup(PP.N_COLS, PP.L, ins_slots=PP.J) as p:
        b.run()
        b.pileup_add(p, sides='origin', col0=np.zeros(b.n, np.int64), mutant_col0=np.zeros(b.n, np.int64))
        b.sync()
        ins = p.ins_counts()
        assert (ins == PP.expected_plane()).all()                         # the construction came out as planted
        p.set_counts(PP.counts())
        yield p, PP.counts(), ins, PP.frame()


@pytest.mark.parametrize('min_depth', (3, 2))
def test_column_polish_from_planted_counts(planted, min_depth):
    from biseqt_amd.batch import DeviceArena
    p, counts, ins, frame = planted
    host = np.concatenate([np.full(16, 9, np.uint8), frame, np.full(16, 9, np.uint8)])
    sets = RC.ordered_read_sets()
    assert [(o, n) for o, n in sets[:8]] == [(o, n) for o, n in PP.read_sets()[:8]]             # the single reads as they are
    with DeviceArena(host) as dev:
        for q, (offs, lens) in enumerate(sets):
            _check(p, frame if q == 4 else (dev, 16), counts, ins, PP.L, frame, offs, lens, min_depth)
        full, _, st = p.polish((dev, 16), [120], [5], min_depth=min_depth, columns=True)
        assert full.tolist() == [0, 1, 2, 3] * 5 and st.tolist() == [(5, 0, 0, 15)]                 # 1 + J letters per column
        assert p.colmap(118, 127).tolist() == [0, 0, 0, 4, 8, 12, 16, 20, 20]
        assert p.polish((dev, 16), [100], [10], min_depth=min_depth, columns=True)[0].size == 0    # every column deleted
        assert not p.colmap().any()
        letters, offsets, stats = p.polish((dev, 16), [], [], columns=True)                         # no reads
        assert letters.size == 0 and offsets.tolist() == [0] and stats.size == 0 and not p.colmap().any()


@pytest.fixture(scope='module')
def wide():
    """1100 columns, eight slots: the plane from the planted pairs of tests/rounds_cases.py, the counts made for that plane."""
    from biseqt_amd.batch import BatchAligner, Pileup
    with BatchAligner(RC.wide_pairs(), alnmode=0, alntype=0, alphabet_len=RC.WIDE_L, **PP.GAPPY) as b, \
            Pileup(RC.WIDE_COLS, RC.WIDE_L, ins_slots=RC.WIDE_J) as p:
        b.run()
        b.pileup_add(p, sides='origin', col0=np.zeros(b.n, np.int64), mutant_col0=np.zeros(b.n, np.int64))
        b.sync()
        ins = p.ins_counts()
        counts, nine = RC.wide_counts(ins)
        assert len(nine) >= 1
        p.set_counts(counts)
        yield p, counts, ins, RC.wide_frame(), nine


@pytest.mark.parametrize('q', range(len(RC.WIDE_READ_SETS)))
def test_reads_across_the_chunks_of_the_grid_and_a_ninth_letter(wide, q):
    p, counts, ins, frame, nine = wide
    offs, lens = RC.WIDE_READ_SETS[q]
    want, wmap = _check(p, frame, counts, ins, RC.WIDE_L, frame, offs, lens, 1)
    e = np.diff(wmap.astype(np.int64))
    inside = np.zeros(RC.WIDE_COLS, bool)
    for o, n in zip(offs, lens):
        inside[o:o + n] = True
    assert not e[~inside].any()                                           # a column that lies in no read emits nothing
    if q < 4:
        assert e.max() == 9 and all(e[c] == 9 for c in nine if inside[c])


def test_column_polish_without_a_plane_and_the_refusals(planted):
    from biseqt_amd import _pwlib as W
    from biseqt_amd.batch import Pileup
    _, counts, _, frame = planted
    lib = W.load()
    out = np.zeros(PP.N_COLS + 1, np.uint64)
    with Pileup(PP.N_COLS, PP.L) as p:
        letters_dev = lib.pw_pileup_counts_device(p.handle)               # (any device pointer: a refused call reads nothing)
        assert not lib.pw_pileup_colmap_device(p.handle) and 'before pw_pileup_polish_columns' in W.last_error()
        assert lib.pw_pileup_colmap(p.handle, 0, 1, out.ctypes.data) == -1 and 'before pw_pileup_polish_columns' in W.last_error()
        p.set_counts(counts)
        for offs, lens in ([0, 100, 110], [100, 10, 0]), ([7, 7, 7, 8], [0, 0, 1, 292]):
            want, wmap = _check(p, frame, counts, None, PP.L, frame, offs, lens, 3)                # no plane: no insertions
        letters, offsets, stats = p.polish(frame, [0, 100, 110], [100, 10, 0], min_depth=3, columns=True)
        assert not stats['inserted'].any()
        kept = (letters.tolist(), offsets.tolist(), stats.tolist(), p.colmap().tolist())

        def refused(offs, lens, why):
            o, n = np.array(offs, np.int64), np.array(lens, np.int32)
            assert lib.pw_pileup_polish_columns(p.handle, letters_dev, o.ctypes.data, n.ctypes.data, len(o), 1, None) == -1
            assert why in W.last_error(), W.last_error()
            # the results of the last polish are still there
            got = np.zeros(len(kept[0]), np.uint8)
            assert lib.pw_pileup_polished_total(p.handle) == len(kept[0])
            assert lib.pw_pileup_polished_letters(p.handle, got.ctypes.data) == 0 and got.tolist() == kept[0]
            assert p.colmap().tolist() == kept[3]

        refused([0, 5], [6, 3], 'read 1 overlaps read 0')
        refused([0, 10, 19], [5, 10, 3], 'read 2 overlaps read 1')
        refused([10, 0], [3, 3], 'read 1 is not in column order')
        refused([0, 20, 10], [0, 0, 0], 'read 2 is not in column order')
        for off, ln in ((298, 3), (-1, 1), (301, 0), (0, -1)):
            refused([off], [ln], 'read 0 lies outside the pileup')
        assert lib.pw_pileup_colmap(p.handle, 0, PP.N_COLS + 2, out.ctypes.data) == -1 and 'outside' in W.last_error()
        assert lib.pw_pileup_colmap(p.handle, 5, 4, out.ctypes.data) == -1
        with pytest.raises(RuntimeError, match='overlaps|column order'):
            p.polish(frame, *PP.read_sets()[8], columns=True)             # the random set of 64 reads overlaps as it comes
        p.polish(frame, [0], [10])                                        # a per-read polish: no map any more
        assert lib.pw_pileup_colmap(p.handle, 0, 1, out.ctypes.data) == -1 and 'before pw_pileup_polish_columns' in W.last_error()
        with pytest.raises(RuntimeError, match='before pw_pileup_polish_columns'):
            p.colmap()
