"""The consensus flow on the device (``OverlapGraph.consensus``, ``assemble_reads(consensus=True)``; include/pw_consensus.h)
against the oracle side of tests/consensus_cases.py on the noisy fixture of tests/test_consensus_ref.py: the oracle gets the
device's own overlap records and CPU-oracle alignments of the tasks, and every comparison is ``==``."""
import numpy as np
import pytest

from tests import consensus_cases as CC
from tests import polish_cases as PC

pytestmark = pytest.mark.gpu


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
    return CC.oracle_consensus(oracle, CC.noisy_fixture()['fx']['reads'], device_graph[1])


def _same(got, records, want):
    assert [len(c) for c in got] == [len(c) for c in want['contigs']]            # (the offsets of the polished letters)
    assert [c.tolist() for c in got] == [c.tolist() for c in want['contigs']]
    assert records.tolist() == want['stats'].tolist()


def test_consensus_equals_the_oracle_letter_for_letter(device_graph, want):
    from biseqt_amd.batch import POLISH_STATS_DTYPE
    G, _ = device_graph
    nf = CC.noisy_fixture()
    stats = {}
    got, records = G.consensus(nf['fx']['reads'], PC.L, PC.COMPLEMENT, slack=CC.SLACK, drift=CC.DRIFT, min_depth=PC.MIN_DEPTH,
                               ins_slots=PC.INS_SLOTS, self_weight=PC.SELF_WEIGHT, stats=stats)
    assert all(c.dtype == np.uint8 for c in got) and records.dtype == POLISH_STATS_DTYPE
    assert G.placements().tolist() == want['places']
    _same(got, records, want)
    placed = sum(p[0] >= 0 for p in want['places'])
    assert (stats['placed'], stats['unplaced'], stats['tasks'], stats['aligned']) == \
        (placed, len(want['places']) - placed, len(want['tasks']), want['aligned'])
    assert all(stats[k] >= 0 for k in ('layout_ms', 'align_ms', 'polish_ms'))
    assert [c.tolist() for c in G.contigs(nf['fx']['reads'], PC.COMPLEMENT)] == [c.tolist() for c in want['draft']]
    before, after = CC.errors(want['draft'], nf['genome']), CC.errors(got, nf['genome'])
    print('contigs %r, tasks %d; errors: draft %d, polished %d' % ([len(c) for c in got], stats['tasks'], before, after))
    assert max(len(c) for c in got) >= len(nf['genome']) // 2 and before >= 40 and 2 * after < before, (before, after)


def test_three_batches_give_the_same_consensus(device_graph, want):
    G, _ = device_graph
    reads = CC.noisy_fixture()['fx']['reads']
    cells = [(t[5] - t[4] + 1) * min(t[3], len(reads[t[2]])) for t in want['tasks']]
    max_cells = sum(cells) // 3 + 1
    assert max(cells) < max_cells and sum(cells) > 2 * max_cells                 # three batches or four
    stats = {}
    got, records = G.consensus(reads, PC.L, PC.COMPLEMENT, slack=CC.SLACK, drift=CC.DRIFT, min_depth=PC.MIN_DEPTH,
                               ins_slots=PC.INS_SLOTS, self_weight=PC.SELF_WEIGHT, max_cells=max_cells, stats=stats)
    _same(got, records, want)
    assert stats['aligned'] == want['aligned']


def test_assemble_reads_with_consensus_from_raw_reads():
    from biseqt_amd.batch import POLISH_STATS_DTYPE
    from biseqt_amd.graph import PLACE_DTYPE
    from biseqt_amd.overlap import assemble_reads
    from biseqt_amd.sequence import Alphabet
    nf = CC.noisy_fixture()
    reads, genome = nf['fx']['reads'], nf['genome']
    kw = dict(p_min=.7, strands='both', complement=PC.COMPLEMENT)
    stats = {}
    contigs, unitigs, members, contained = assemble_reads(reads, 10, Alphabet('ACGT'), .2, .9, consensus=True, stats=stats, **kw)
    draft = stats['draft']
    assert len(contigs) == len(draft) == len(unitigs) == len(stats['consensus_records'])
    assert stats['consensus_records'].dtype == POLISH_STATS_DTYPE and stats['placements'].dtype == PLACE_DTYPE
    assert len(stats['placements']) == len(reads) and all(stats[k] >= 0 for k in ('layout_ms', 'consensus_align_ms', 'polish_ms'))
    before, after = CC.errors(draft, genome), CC.errors(contigs, genome)
    print('assemble_reads: contigs %r -> %r, %r; errors: draft %d, polished %d'
          % ([len(c) for c in draft], [len(c) for c in contigs], stats['consensus_stats'], before, after))
    assert 2 * after < before, (before, after)
    plain = assemble_reads(reads, 10, Alphabet('ACGT'), .2, .9, **kw)
    assert [c.tolist() for c in plain[0]] == [c.tolist() for c in draft]
    assert plain[1].tolist() == unitigs.tolist() and plain[2].tolist() == members.tolist() and plain[3].tolist() == contained.tolist()
