"""The overlap graph fed by the aligner: ``OverlapGraph.add_batch`` on a real banded-overlap batch against records computed
on the host from the batch's results and summaries, ``overlap_alignments(graph=...)`` against the same records added by
hand, and ``assemble_reads`` from raw reads against tests/graph_ref.py fed with the records the device produced."""
import numpy as np
import pytest

from tests import graph_cases as GC
from tests import graph_ref as R

pytestmark = pytest.mark.gpu

SCORES = dict(match_score=1, mismatch_score=-3, go_score=-5, ge_score=-2)
FIELDS = ('a', 'b', 'strand', 'a_beg', 'a_end', 'b_beg', 'b_end', 'n_match', 'n_ops')


def _rows(recs):
    return [tuple(int(r[f]) for f in FIELDS) for r in recs]


@pytest.fixture(scope='module')
def overlapping_reads():
    """14 error-free reads over 1500 letters on both strands; the pairs that truly overlap, each with a band around its
    diagonal, and two pairs whose band is empty (``dmax == dmin - 1``): the batch plans them as tables without a cell and they
    get no alignment."""
    _, reads, recs = GC.linear(5, n_reads=14, genome_len=1500)
    lens = [len(r) for r in reads]
    have = set((r[0], r[1]) for r in recs)
    spare = [(a, b) for a in range(14) for b in range(a + 1, 14) if (a, b) not in have][:2]
    assert len(spare) == 2
    pairs = [(r[0], r[1]) for r in recs] + spare
    strands = [r[2] for r in recs] + [0, 1]
    bands = []
    for r in recs:
        d = r[3] - r[5]
        bands.append((max(d - 8, -lens[r[1]]), min(d + 8, lens[r[0]])))
    bands += [(10, 9), (-3, -4)]
    assert 30 <= len(recs) <= 60 and 0 in strands[:-2] and 1 in strands[:-2]
    return reads, lens, np.array(pairs, np.int64), np.array(strands, np.uint8), np.array(bands, np.int64), recs


def _host_records(pairs, strands, res, sums):
    rows = []
    for k in range(len(pairs)):
        row = [int(pairs[k, 0]), int(pairs[k, 1]), int(strands[k]), 0, 0, 0, 0, 0, 0]
        if sums['flags'][k] & 1:
            s = sums[k]
            row[3] = int(res['origin_idx'][k]); row[4] = row[3] + int(s['n_match'] + s['n_subst'] + s['n_del'])
            row[5] = int(res['mutant_idx'][k]); row[6] = row[5] + int(s['n_match'] + s['n_subst'] + s['n_ins'])
            row[7] = int(s['n_match']); row[8] = int(s['n_match'] + s['n_subst'] + s['n_ins'] + s['n_del'])
        rows.append(tuple(row))
    return rows


def test_add_batch_equals_the_records_computed_on_the_host(overlapping_reads):
    from biseqt_amd.batch import pack_reads
    from biseqt_amd.graph import OverlapGraph
    from biseqt_amd.overlap import aligned_batches
    reads, lens, pairs, strands, bands, true_recs = overlapping_reads
    arena, offs, rlens = pack_reads(reads)
    batches = 0
    with OverlapGraph(lens) as G:
        for start, stop, b in aligned_batches(arena, offs, rlens, pairs, bands, 4, strands=strands, complement=GC.COMPLEMENT, check_band=False,
                                          **SCORES):
            batches += 1
            assert (start, stop) == (0, len(pairs))
            G.add_batch(b, pairs[:, 0], pairs[:, 1], strands)          # summarises by itself: no summary was taken yet
            res, sums = b.results(), b.summaries()
            want = _host_records(pairs, strands, res, sums)
            assert _rows(G.overlaps()) == want
            assert [w[8] == 0 for w in want[-2:]] == [True, True]       # a table without a cell: no alignment
            wrong = pairs[:, 0].copy()
            wrong[0] = [r for r in range(14) if lens[r] != lens[pairs[0, 0]] and r != pairs[0, 1]][0]
            with pytest.raises(RuntimeError, match='whole reads'):
                G.add_batch(b, wrong, pairs[:, 1], strands)
            with pytest.raises(RuntimeError, match='itself'):
                G.add_batch(b, pairs[:, 1], pairs[:, 1], strands)
            with pytest.raises(ValueError):
                G.add_batch(b, pairs[:-1, 0], pairs[:-1, 1], strands[:-1])
            assert len(G) == len(pairs)                                 # a refused call appends nothing
            G.build(min_overlap=20)
            got = GC.snapshot(G)
            assert got == R.build(lens, want, min_overlap=20)
            assert got['cls'][-2:] == [R.NONE, R.NONE] and R.NONE not in got['cls'][:-2]
    assert batches == 1


def test_overlap_alignments_feeds_an_open_graph(overlapping_reads):
    from biseqt_amd.graph import OverlapGraph
    from biseqt_amd.overlap import overlap_alignments
    from biseqt_amd.sequence import Alphabet
    reads, lens, pairs, strands, bands, true_recs = overlapping_reads
    pairs, strands, bands = pairs[:len(true_recs)], strands[:len(true_recs)], bands[:len(true_recs)]
    plist = [tuple(p) for p in pairs.tolist()]
    blist = [dict(p=1., d_band=tuple(d)) for d in bands.tolist()]
    blist[1] = None                                                     # a pair without a band is not aligned: no record
    sl = ['-' if s else '+' for s in strands.tolist()]
    snaps = []
    for kw in (dict(want_transcripts=False, max_cells=40000), dict(want_transcripts=True)):
        with OverlapGraph(lens) as G:
            alns = overlap_alignments(reads, plist, blist, Alphabet('ACGT'), strands=sl, complement=GC.COMPLEMENT, graph=G, **kw)
            assert len(G) == len(plist) - 1 and alns[1] is None
            recs = G.overlaps()
            assert [(int(r['a']), int(r['b']), int(r['strand'])) for r in recs] == \
                [(p[0], p[1], int(s)) for q, (p, s) in enumerate(zip(plist, strands.tolist())) if q != 1]
            G.build(min_overlap=20)
            snaps.append((_rows(recs), GC.snapshot(G)))
    assert snaps[0] == snaps[1]
    rows, snap = snaps[0]
    assert GC.device_build(lens, rows, min_overlap=20) == snap          # the same records added by hand: the same graph
    assert snap == R.build(lens, rows, min_overlap=20)
    with pytest.raises(ValueError, match='graph'):
        with OverlapGraph(lens[:-1]) as G:
            overlap_alignments(reads, plist, blist, Alphabet('ACGT'), strands=sl, complement=GC.COMPLEMENT, graph=G)


def test_assemble_reads_from_raw_reads_on_both_strands():
    """wordlen 12 on 6000 random letters leaves a few chance seeds and no chance band with p >= .8; whatever chance overlap
    came through all the same would be a handful of letters long, and min_overlap = 60 classes it WEAK."""
    from biseqt_amd.overlap import assemble_reads
    from biseqt_amd.sequence import Alphabet
    genome, reads, _ = GC.linear(4, n_reads=120)
    lens = [len(r) for r in reads]
    stats = {}
    params = dict(min_overlap=60, fuzz=10)
    contigs, unitigs, members, contained = assemble_reads(reads, 12, Alphabet('ACGT'), .2, .9, p_min=.8, strands='both',
                                                          complement=GC.COMPLEMENT, stats=stats, **params)
    rows = _rows(stats['records'])
    assert stats['aligned'] > 100 and len(rows) >= stats['aligned']
    want = R.build(lens, rows, **params)
    assert stats['records']['cls'].tolist() == want['cls']
    assert contained.tolist() == want['contained']
    assert unitigs[['first_member', 'length', 'n_members', 'head', 'circular']].tolist() == want['unitigs']
    assert members.tolist() == want['members']
    assert stats['arcs'] == len(want['arcs']) and stats['kept_arcs'] == sum(1 for a in want['arcs'] if not a[5] & R.REMOVED)
    assert all(stats[k] >= 0 for k in ('overlap_ms', 'align_ms', 'build_ms', 'contigs_ms')) and stats['device_bytes'] > 0
    letters = R.contigs(reads, want['unitigs'], want['members'], GC.COMPLEMENT)
    whole = (genome.tobytes(), GC.rc(genome).tobytes())
    for c in letters:                                                   # the oracle's side first: a failure says which side broke it
        assert bytes(bytearray(c)) in whole[0] or bytes(bytearray(c)) in whole[1]
    assert [c.tolist() for c in contigs] == letters
    for c in contigs:
        assert c.tobytes() in whole[0] or c.tobytes() in whole[1]
    print('assemble_reads: %d records, %d arcs (%d kept), %d unitigs, longest contig %d'
          % (len(rows), stats['arcs'], stats['kept_arcs'], len(unitigs), max(len(c) for c in contigs)))
