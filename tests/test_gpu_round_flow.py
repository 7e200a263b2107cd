"""The iterated consensus on the device (``OverlapGraph.consensus(rounds=k)``, ``assemble_reads(consensus_rounds=k)``;
include/pw_rounds.h) against the oracle side of tests/rounds_ref.py on the noisy fixture of tests/consensus_cases.py: the
oracle gets the device's own overlap records and CPU-oracle alignments of every round's tasks, and every comparison is ``==``.

On the oracle's own records (tests/test_rounds_ref.py) the rounds leave 14, 11, 10 and 10 errors against the genome and
stop behind round 4, which changes nothing."""
import pytest

from tests import consensus_cases as CC
from tests import graph_cases as GC
from tests import polish_cases as PC
from tests import rounds_ref as RR

pytestmark = pytest.mark.gpu
KW = dict(slack=CC.SLACK, drift=CC.DRIFT, min_depth=PC.MIN_DEPTH, ins_slots=PC.INS_SLOTS, self_weight=PC.SELF_WEIGHT)


@pytest.fixture(scope='module')
def device_graph():
    """The fixture's pairs aligned on the device into a graph, built: (graph, its records as tuples)."""
    from biseqt_amd.graph import OverlapGraph
    from biseqt_amd.overlap import overlap_alignments
    from biseqt_amd.sequence import Alphabet
    fx = CC.noisy_fixture()['fx']
    with OverlapGraph([len(r) for r in fx['reads']]) as G:
        overlap_alignments(fx['reads'], fx['pairs'], fx['bands'], Alphabet('ACGT'), strands=fx['strands'], complement=PC.COMPLEMENT,
                           want_transcripts=False, graph=G)
        G.build()
        recs = G.overlaps()
        fields = ('a', 'b', 'strand', 'a_beg', 'a_end', 'b_beg', 'b_end', 'n_match', 'n_ops')
        yield G, [tuple(int(r[f]) for f in fields) for r in recs]


@pytest.fixture(scope='module')
def want(device_graph, oracle):
    """The oracle's rounds, computed once: asked for five, it stops behind the first round that changes nothing."""
    return RR.oracle_rounds(oracle, CC.noisy_fixture()['fx']['reads'], device_graph[1], 5)[1]


def _fixed(r):
    return not (r['stats']['substituted'].any() or r['stats']['deleted'].any() or r['stats']['inserted'].any())


def _same(got, records, stats, want, k):
    ran = min(k, len(want))
    w = want[ran - 1]
    assert [len(c) for c in got] == [len(c) for c in w['contigs']]
    assert [c.tolist() for c in got] == [c.tolist() for c in w['contigs']]
    assert records.tolist() == w['stats'].tolist()
    assert len(stats['rounds']) == ran
    for r, wr in zip(stats['rounds'], want):
        assert (r['tasks'], r['aligned'], r['records'].tolist()) == (len(wr['tasks']), wr['aligned'], wr['stats'].tolist())
        assert all(r[key] >= 0 for key in ('layout_ms', 'align_ms', 'polish_ms'))
    assert (stats['tasks'], stats['aligned']) == (len(w['tasks']), w['aligned'])
    assert all(abs(stats[key] - sum(r[key] for r in stats['rounds'])) < 1e-6 for key in ('layout_ms', 'align_ms', 'polish_ms'))


@pytest.mark.parametrize('k', (2, 3, 5))
def test_rounds_equal_the_oracle_letter_for_letter(device_graph, want, k):
    G, _ = device_graph
    nf = CC.noisy_fixture()
    assert len(want) == 4 and _fixed(want[3]) and not any(_fixed(r) for r in want[:3])       # five asked for: four run
    stats = {}
    got, records = G.consensus(nf['fx']['reads'], PC.L, PC.COMPLEMENT, stats=stats, rounds=k, **KW)
    _same(got, records, stats, want, k)
    assert G.round() == min(k, 4) and G.lengths().tolist() == [len(c) for c in want[min(k, 4) - 2]['contigs']]
    assert G.placements().tolist() == want[0]['places']
    errors = [CC.errors(r['contigs'], nf['genome']) for r in want[:min(k, 4)]]
    print('rounds %d: contigs %r, errors against the genome per round %r' % (k, [len(c) for c in got], errors))
    assert CC.errors(got, nf['genome']) == errors[-1] <= errors[0]


def test_one_round_is_the_consensus_of_today(device_graph, want):
    G, _ = device_graph
    reads = CC.noisy_fixture()['fx']['reads']
    s0, s1 = {}, {}
    plain, precords = G.consensus(reads, PC.L, PC.COMPLEMENT, stats=s0, **KW)
    got, records = G.consensus(reads, PC.L, PC.COMPLEMENT, stats=s1, rounds=1, **KW)
    assert [c.tolist() for c in got] == [c.tolist() for c in plain] and records.tolist() == precords.tolist()
    _same(got, records, s1, want, 1)
    today = {'placed', 'unplaced', 'tasks', 'aligned', 'layout_ms', 'align_ms', 'polish_ms'}
    assert today <= set(s0) and set(s0) == set(s1) and all(s0[key] == s1[key] for key in ('placed', 'unplaced', 'tasks', 'aligned'))
    assert G.round() == 1
    with pytest.raises(ValueError):
        G.consensus(reads, PC.L, PC.COMPLEMENT, rounds=0, **KW)


def test_three_batches_a_round_give_the_same_letters(device_graph, want):
    G, _ = device_graph
    reads = CC.noisy_fixture()['fx']['reads']
    cells = [(t[5] - t[4] + 1) * min(t[3], len(reads[t[2]])) for t in want[0]['tasks']]
    max_cells = sum(cells) // 3 + 1
    assert max(cells) < max_cells and sum(cells) > 2 * max_cells                 # three batches or four
    stats = {}
    got, records = G.consensus(reads, PC.L, PC.COMPLEMENT, max_cells=max_cells, stats=stats, rounds=3, **KW)
    _same(got, records, stats, want, 3)


def test_error_free_reads_reach_the_fixed_point_at_once():
    from biseqt_amd.graph import OverlapGraph
    _, reads, records, _ = CC.chains()
    with OverlapGraph([len(r) for r in reads]) as G:
        G.add(records)
        G.build()
        draft = G.contigs(reads, GC.COMPLEMENT)
        stats = {}
        got, recs = G.consensus(reads, 4, GC.COMPLEMENT, stats=stats, rounds=4)
        assert len(stats['rounds']) == 1 and G.round() == 1
        assert [c.tolist() for c in got] == [c.tolist() for c in draft]
        assert recs['kept'].tolist() == [len(c) for c in draft] and not (recs['substituted'].any() or recs['deleted'].any() or recs['inserted'].any())


def test_assemble_reads_with_rounds_from_raw_reads_equals_the_graph_call():
    from biseqt_amd.graph import OverlapGraph
    from biseqt_amd.overlap import assemble_reads
    from biseqt_amd.sequence import Alphabet
    nf = CC.noisy_fixture()
    reads, genome = nf['fx']['reads'], nf['genome']
    stats = {}
    contigs, unitigs, _, _ = assemble_reads(reads, 10, Alphabet('ACGT'), .2, .9, consensus=True, consensus_rounds=2, stats=stats,
                                            p_min=.7, strands='both', complement=PC.COMPLEMENT)
    assert len(stats['consensus_rounds']) == 2 and len(contigs) == len(unitigs) == len(stats['consensus_records'])
    with OverlapGraph([len(r) for r in reads]) as G:
        G.add(stats['records'])
        G.build()
        gstats = {}
        got, records = G.consensus(reads, 4, PC.COMPLEMENT, rounds=2, stats=gstats)
    assert [c.tolist() for c in got] == [c.tolist() for c in contigs] and records.tolist() == stats['consensus_records'].tolist()
    assert [r['records'].tolist() for r in gstats['rounds']] == [r['records'].tolist() for r in stats['consensus_rounds']]
    before, after = CC.errors(stats['draft'], genome), CC.errors(contigs, genome)
    print('assemble_reads, two rounds: contigs %r; errors: draft %d, polished %d' % ([len(c) for c in contigs], before, after))
    assert 2 * after < before, (before, after)
