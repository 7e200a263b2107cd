"""Contig letters on the device against tests/graph_ref.py: the letters, and with them the offsets and totals, of the planted
cases; letters given as a host array and as a view of a device arena; letters outside the alphabet; the call order."""
import numpy as np
import pytest

from tests import graph_cases as GC
from tests import graph_ref as R

pytestmark = pytest.mark.gpu

CASES = {
    'ring 12': lambda: GC.ring(12),
    'ring 65': lambda: GC.ring(65),
    'linear 150': lambda: GC.linear(1),
    'linear 60, several unitigs': lambda: GC.linear(3, n_reads=60),
    'chain 33': lambda: GC.ladder(33, 100, 60, both_strands=True),
    'ladder': lambda: GC.ladder(100, 400, 5, both_strands=True),
}


@pytest.fixture(scope='module', params=sorted(CASES))
def case(request):
    genome, reads, recs = CASES[request.param]()
    want = R.build([len(r) for r in reads], recs)
    return request.param, genome, reads, recs, want, R.contigs(reads, want['unitigs'], want['members'], GC.COMPLEMENT)


def test_contig_letters_from_host_reads_and_from_a_device_arena(case):
    from biseqt_amd.batch import DeviceArena, pack_reads
    from biseqt_amd.graph import OverlapGraph
    name, genome, reads, recs, want, letters = case
    with OverlapGraph([len(r) for r in reads]) as G:
        G.add(recs)
        G.build()
        got = G.contigs(reads, GC.COMPLEMENT)
        assert [c.tolist() for c in got] == letters
        assert [len(c) for c in got] == [u[1] for u in want['unitigs']]
        assert int(G.lib.pw_graph_contig_total(G.handle)) == sum(u[1] for u in want['unitigs'])
        arena, offs, _ = pack_reads(reads)
        with DeviceArena(arena) as dev:
            assert [c.tolist() for c in G.contigs((dev, offs), GC.COMPLEMENT)] == letters
            with pytest.raises(ValueError):
                G.contigs((dev, offs[:-1]), GC.COMPLEMENT)
    whole = (genome.tobytes(), GC.rc(genome).tobytes())
    for c in got:
        if name.startswith('ring'):
            assert GC.is_rotation(c, genome) or GC.is_rotation(c, GC.rc(genome))
        else:
            assert c.tobytes() in whole[0] or c.tobytes() in whole[1]


def test_letters_outside_the_alphabet_stay_what_they_are():
    from biseqt_amd.graph import OverlapGraph
    _, reads, recs = GC.ladder(9, 100, 60, both_strands=True)
    reads = [r.copy() for r in reads]
    for k, r in enumerate(reads):
        r[[3, 50, 97]] = (4, 200, 255)[k % 3]
    want = R.build([100] * 9, recs)
    assert any(m[0] & 1 for m in want['members'])
    with OverlapGraph([100] * 9) as G:
        G.add(recs)
        G.build()
        got = G.contigs(reads, GC.COMPLEMENT)
        assert [c.tolist() for c in got] == R.contigs(reads, want['unitigs'], want['members'], GC.COMPLEMENT)
        assert {4, 200, 255} & set(got[0].tolist())
        with pytest.raises(ValueError, match='complement'):
            G.contigs(reads)                               # a reverse-complemented member and no table


def test_forward_members_need_no_complement():
    from biseqt_amd.graph import OverlapGraph
    genome, reads, recs = GC.ladder(5, 100, 60)
    with OverlapGraph([100] * 5) as G:
        G.add(recs)
        G.build()
        (contig,) = G.contigs(reads)
        assert contig.tobytes() == genome.tobytes()


def test_contigs_before_build_and_after_a_rebuild():
    from biseqt_amd.graph import OverlapGraph
    _, reads, recs = GC.ladder(5, 100, 60)
    with OverlapGraph([100] * 5) as G:
        G.add(recs)
        with pytest.raises(RuntimeError, match='before pw_graph_build'):
            G.contigs(reads, GC.COMPLEMENT)
        assert int(G.lib.pw_graph_contig_total(G.handle)) == -1
        G.build()
        assert int(G.lib.pw_graph_contig_total(G.handle)) == -1         # ... and before the first pw_graph_contigs
        assert len(G.contigs(reads, GC.COMPLEMENT)) == 1
        G.build(min_overlap=80)                                         # every overlap is weak now: five unitigs of one
        assert int(G.lib.pw_graph_contig_total(G.handle)) == -1         # the rebuild drops the letters
        assert [c.tolist() for c in G.contigs(reads, GC.COMPLEMENT)] == [r.tolist() for r in reads]
