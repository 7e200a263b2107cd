"""Cleaning from raw reads: ``assemble_reads`` on a tiled genome plus two reads whose last third is random letters, against
tests/graph_clean_ref.py fed with the records the device produced.

The inputs (tests/graph_clean_cases.py, ``junk_tails``): 3000 letters tiled by 27 error-free reads of 400 at every 100, on
alternating strands, and two more reads at 250 (stored forwards) and 1450 (stored reverse-complemented), off the grid so that
no read contains them, whose last 133 letters as stored are random.  With CPU-oracle overlap alignments of every pair that
shares 30 letters or more (banded B_OVERLAP, 1 / -3 / -5 / -2, 16 diagonals either side), ``min_overlap = 60`` and
``min_identity = .9``, each planted read keeps two clean dovetails into its good end (150 and 250 letters, identity 1) and
every overlap that runs into its junk has identity .52 .. .89 and is WEAK: a one-read dead end on the line.  The oracle then
gives five unitigs (2, 14, 11, 1, 1 reads) without cleaning and one of 27 reads with ``max_tip_reads = 2``, reads 27 and 28
dropped and placed at 250 and 1450.  (With ``min_identity = 0`` the junk overlaps are dovetails and the planted reads become
members: that is why the identity bound is part of the case.)"""
import pytest

from tests import graph_cases as GC
from tests import graph_clean_cases as CC
from tests import graph_clean_ref as K
from tests import graph_ref as R

pytestmark = pytest.mark.gpu

FIELDS = ('a', 'b', 'strand', 'a_beg', 'a_end', 'b_beg', 'b_end', 'n_match', 'n_ops')
PARAMS = dict(min_overlap=60, min_identity=.9, fuzz=10)


def _assemble(reads, **kw):
    from biseqt_amd.overlap import assemble_reads
    from biseqt_amd.sequence import Alphabet
    stats = {}
    out = assemble_reads(reads, 12, Alphabet('ACGT'), .2, .9, p_min=.8, strands='both', complement=GC.COMPLEMENT, stats=stats,
                         **dict(PARAMS, **kw))
    return out, stats, [tuple(int(r[f]) for f in FIELDS) for r in stats['records']]


def test_two_junk_tailed_reads_break_the_line_and_cleaning_mends_it():
    genome, reads, planted, _ = CC.junk_tails()
    lens = [len(r) for r in reads]
    whole = (genome.tobytes(), GC.rc(genome).tobytes())
    # ---- without cleaning: the line is broken ----
    (contigs, unitigs, members, contained), stats, rows = _assemble(reads)
    want = K.build(lens, rows, **PARAMS)
    assert want == dict(R.build(lens, rows, **PARAMS), dropped=[0] * len(lens))
    assert stats['records']['cls'].tolist() == want['cls'] and stats['dropped']['reads'].tolist() == want['dropped']
    assert unitigs[['first_member', 'length', 'n_members', 'head', 'circular']].tolist() == want['unitigs']
    assert (stats['dropped']['tips'], stats['dropped']['bubbles']) == (0, 0)
    assert len(unitigs) > 1
    # ---- with it: exactly the two planted reads go, and one unitig remains ----
    (contigs, unitigs, members, contained), stats, rows2 = _assemble(reads, max_tip_reads=2)
    assert rows2 == rows
    want = K.build(lens, rows, max_tip_reads=2, **PARAMS)
    assert [r for r, d in enumerate(want['dropped']) if d] == planted            # the oracle's side first
    assert stats['records']['cls'].tolist() == want['cls'] and contained.tolist() == want['contained']
    assert stats['dropped']['reads'].tolist() == want['dropped']
    assert (stats['dropped']['tips'], stats['dropped']['bubbles']) == (2, 0)
    assert unitigs[['first_member', 'length', 'n_members', 'head', 'circular']].tolist() == want['unitigs']
    assert members.tolist() == want['members']
    assert stats['kept_arcs'] == sum(1 for a in want['arcs'] if not a[5] & K.REMOVED)
    assert len(unitigs) == 1 and int(unitigs['n_members'][0]) == len(reads) - 2
    assert [c.tolist() for c in contigs] == R.contigs(reads, want['unitigs'], want['members'], GC.COMPLEMENT)
    assert contigs[0].tobytes() in whole[0] or contigs[0].tobytes() in whole[1]


def test_with_the_consensus_the_dropped_reads_are_placed():
    genome, reads, planted, _ = CC.junk_tails()
    lens = [len(r) for r in reads]
    (contigs, unitigs, members, contained), stats, rows = _assemble(reads, max_tip_reads=2, consensus=True)
    want = K.build(lens, rows, max_tip_reads=2, **PARAMS)
    places = stats['placements'][['unitig', 'rev', 'pos', 'root', 'depth']].tolist()
    assert places == K.place(lens, rows, want)
    assert all(places[r][0] == 0 and places[r][4] == 1 for r in planted)
    assert stats['consensus_stats']['unplaced'] == 0 and stats['consensus_stats']['placed'] == len(reads) and len(contigs) == 1
