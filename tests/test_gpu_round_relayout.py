"""The relayout (``OverlapGraph.consensus_relayout``, ``positions``, ``lengths``; include/pw_rounds.h, pw_rounds.hip) against
the oracle of tests/rounds_ref.py on the planted graphs of tests/test_gpu_consensus_place.py and hand-made polished sets
(tests/rounds_cases.py), uploaded as plain arrays: positions, lengths, contig starts, every field of every task and every
byte of the arena are compared with ``==``, round after round."""
import numpy as np
import pytest

from tests import consensus_cases as CC
from tests import consensus_ref as CR
from tests import graph_cases as GC
from tests import graph_ref as GR
from tests import rounds_cases as RC
from tests import rounds_ref as RR

pytestmark = pytest.mark.gpu


def _ring_with_contained():
    _, reads, records = GC.ring(seed=3)
    n = len(reads)
    for r in range(0, n, 2):
        reads.append(reads[r][100:300].copy())
        records.append((r, n + r // 2, 0, 100, 300, 0, 200, 200, 200))
    return reads, sorted(records)


def _past_the_ends():
    """The 'edges' case with two grandchildren: read 13 lies in read 9, which only touches the contig's end, and read 14 in
    read 4, which only touches its start -- so that 13 begins PAST the contig's end and 14 ends before its start."""
    reads, records = CC.planted()['edges']
    reads = list(reads) + [np.full(20, 1, np.uint8), np.full(24, 2, np.uint8)]
    return reads, sorted(list(records) + [(13, 9, 0, 0, 20, 10, 30, 20, 20), (4, 14, 1, 5, 29, 0, 24, 24, 24)])


CASES = {
    'chains': lambda: CC.chains()[1:3],
    'tie': lambda: CC.planted()['tie'],
    'cycles': lambda: CC.planted()['cycles'],
    'edges': lambda: CC.planted()['edges'],
    'past the ends': _past_the_ends,
    'no arcs': lambda: CC.planted()['no_arcs'],
    'ring with contained reads': _ring_with_contained,
    'no reads': lambda: ([], []),
}
SLACK, DRIFT = 7, .25
# the branches of the remap that a case must take (pos against the contig's length n), asserted where the case runs
BRANCHES = {'edges': {'<0', '0', '<n', 'n'}, 'past the ends': {'<0', '0', '<n', 'n', '>n'}, 'chains': {'0', '<n'}}


def _oracle_layout(reads, records):
    lens = [len(r) for r in reads]
    built = GR.build(lens, records)
    places = CR.place(lens, records, built)
    draft = [np.array(c, np.uint8) for c in GR.contigs(reads, built['unitigs'], built['members'], GC.COMPLEMENT)]
    tasks, cstart, nbytes = CR.tasks(lens, places, built['unitigs'], SLACK, DRIFT)
    return lens, dict(places=places, lengths=[u[1] for u in built['unitigs']], tasks=tasks, cstart=cstart, arena_bytes=nbytes,
                      arena=CR.arena(reads, draft, tasks, cstart, nbytes, GC.COMPLEMENT)), draft


def _same(G, got, want):
    cstart, tasks, arena = got
    assert cstart.tolist() == want['cstart'] and tasks.tolist() == want['tasks'] and arena.nbytes == want['arena_bytes']
    assert (arena.read(0, arena.nbytes) == want['arena']).all()
    assert G.positions().tolist() == [p[2] for p in want['places']] and G.lengths().tolist() == want['lengths']
    assert int(G.lib.pw_graph_cons_num_cols(G.handle)) == want['cstart'][-1]
    assert all(t[0] % 4 == 0 and t[1] % 16 == 0 for t in want['tasks'])


@pytest.mark.parametrize('name', sorted(CASES))
def test_relayouts_equal_the_oracle(name):
    from biseqt_amd.graph import OverlapGraph
    reads, records = CASES[name]()
    lens, lay, draft = _oracle_layout(reads, records)
    with OverlapGraph(lens) as G:
        if records:
            G.add(records)
        G.build()
        placements = G.placements().tolist()
        assert placements == lay['places']
        seen = set()
        for variant in RC.VARIANTS:
            first = G.consensus_layout(reads, GC.COMPLEMENT, slack=SLACK, drift=DRIFT)       # round 1 again
            assert G.round() == 1
            _same(G, first, lay)
            cur, contigs = lay, draft
            # two relayouts in a row: the hand-made set, then a random one on top of it
            for k, v in enumerate((variant, 'random')):
                for (u, _, pos, _, _) in cur['places']:
                    if u >= 0:
                        n = cur['lengths'][u]
                        seen.add('<0' if pos < 0 else '0' if pos == 0 else '<n' if pos < n else 'n' if pos == n else '>n')
                contigs, letters, offsets, colmap = RC.polished_set(v, contigs, cur['lengths'], cur['cstart'], seed=k)
                want = RR.next_round(lens, cur['places'], cur['lengths'], cur['cstart'], colmap, contigs, reads, SLACK, DRIFT,
                                     GC.COMPLEMENT)
                got = G.consensus_relayout(letters, offsets, colmap, reads, GC.COMPLEMENT, slack=SLACK, drift=DRIFT)
                assert G.round() == k + 2
                _same(G, got, want)
                if variant == 'identity' and k == 0:                                         # the draft itself: the layout's own
                    assert want['tasks'] == lay['tasks'] and (want['arena'] == lay['arena']).all() and want['cstart'] == lay['cstart']
                if variant == 'first contig empty' and k == 0 and lens:
                    assert want['lengths'][0] == 0 and all(want['places'][t[2]][0] != 0 for t in want['tasks'])
                cur = want
            assert G.placements().tolist() == placements                                    # the build's placements stay
        assert seen >= BRANCHES.get(name, set()), seen
    if name == 'no arcs':                # 37 letters: one more stays below the 4-byte boundary, four more cross it
        l1, l4 = ([n + k for n in lay['lengths']] for k in (1, 4))
        assert CR.contig_starts([(0, n) for n in l1])[1] == lay['cstart'][1] and CR.contig_starts([(0, n) for n in l4])[1] == lay['cstart'][1] + 4


def test_rounds_count_up_and_the_refusals():
    from biseqt_amd import _pwlib as W
    from biseqt_amd.graph import OverlapGraph
    reads, records = CC.planted()['no_arcs']
    lens, lay, draft = _oracle_layout(reads, records)
    out = np.zeros(64, np.int64)
    with OverlapGraph(lens) as G:
        lib, h = G.lib, G.handle

        def nothing_laid_out():
            assert lib.pw_graph_cons_round(h) == -1 and 'before pw_graph_consensus_layout' in W.last_error()
            for f in ('pw_graph_cons_positions', 'pw_graph_cons_lengths'):
                assert getattr(lib, f)(h, out.ctypes.data) == -1 and 'before pw_graph_consensus_layout' in W.last_error()
            with pytest.raises(RuntimeError, match='before pw_graph_consensus_layout'):
                G.consensus_relayout(np.zeros(4, np.uint8), np.zeros(5, np.uint64), np.zeros(5, np.uint64), reads, GC.COMPLEMENT)

        G.build()
        nothing_laid_out()
        G.placements()
        nothing_laid_out()                                                                   # placed, not laid out
        G.consensus_layout(reads, GC.COMPLEMENT, slack=SLACK, drift=DRIFT)
        assert G.round() == 1 and G.lengths().tolist() == lay['lengths'] and G.positions().tolist() == [p[2] for p in lay['places']]
        ident = RC.polished_set('identity', draft, lay['lengths'], lay['cstart'])
        for k in range(2, 5):
            G.consensus_relayout(ident[1], ident[2], ident[3], reads, GC.COMPLEMENT, slack=SLACK, drift=DRIFT)
            assert G.round() == k
        for bad in (dict(slack=-1), dict(drift=-.5), dict(drift=float('nan'))):
            with pytest.raises(ValueError):
                G.consensus_relayout(ident[1], ident[2], ident[3], reads, GC.COMPLEMENT, **bad)
        assert G.round() == 4                                                                # a refused argument changes nothing
        G.consensus_layout(reads, GC.COMPLEMENT, slack=SLACK, drift=DRIFT)                    # a layout is round 1 again
        assert G.round() == 1
        G.consensus_relayout(ident[1], ident[2], ident[3], reads, GC.COMPLEMENT, slack=SLACK, drift=DRIFT)
        assert G.round() == 2
        G.contigs(reads, GC.COMPLEMENT)                                                      # new contig letters drop the layout
        nothing_laid_out()
        G.consensus_layout(reads, GC.COMPLEMENT, slack=SLACK, drift=DRIFT)
        G.consensus_relayout(ident[1], ident[2], ident[3], reads, GC.COMPLEMENT, slack=SLACK, drift=DRIFT)
        # offsets that disagree with the map about a contig's length: refused, and no layout is left
        wrong = ident[2].copy()
        wrong[1:] += 1
        with pytest.raises(RuntimeError, match='disagree with colmap'):
            G.consensus_relayout(np.concatenate([ident[1], [0]]).astype(np.uint8), wrong, ident[3], reads, GC.COMPLEMENT, slack=SLACK,
                                 drift=DRIFT)
        nothing_laid_out()
        G.consensus_layout(reads, GC.COMPLEMENT, slack=SLACK, drift=DRIFT)
        assert G.round() == 1 and G.positions().tolist() == [p[2] for p in lay['places']]
        G.build()                                                                            # a rebuild drops everything
        nothing_laid_out()
        assert len(G.consensus_layout(reads, GC.COMPLEMENT, slack=SLACK, drift=DRIFT)[1]) == len(lay['tasks']) and G.round() == 1
