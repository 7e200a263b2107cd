"""Placements, tasks, contig starts and the consensus arena on the device (include/pw_consensus.h; pw_consensus.hip) against
the oracle of tests/consensus_ref.py on planted records: every field of every record and every byte of the arena is compared
with ``==``.  The cases (tests/consensus_cases.py, asserted by tests/test_consensus_ref.py to hold what they are for):
containment chains of 1, 2, 3, 4, 5, 8 and 9 links on mixed strands, a parent tie, cycles of two and three, reads that stick
out of their contig or miss it, zero-length reads, a circular unitig, a build without arcs, no reads at all, the accessors
before their stage and after a rebuild."""
import numpy as np
import pytest

from tests import consensus_cases as CC
from tests import consensus_ref as CR
from tests import graph_cases as GC
from tests import graph_ref as GR

pytestmark = pytest.mark.gpu


def _ring_with_contained():
    _, reads, records = GC.ring(seed=3)
    n = len(reads)
    for r in range(0, n, 2):
        reads.append(reads[r][100:300].copy())
        records.append((r, n + r // 2, 0, 100, 300, 0, 200, 200, 200))
    return reads, sorted(records)


CASES = {
    'chains': lambda: CC.chains()[1:3],
    'tie': lambda: CC.planted()['tie'],
    'cycles': lambda: CC.planted()['cycles'],
    'edges': lambda: CC.planted()['edges'],
    'no arcs': lambda: CC.planted()['no_arcs'],
    'ring': lambda: GC.ring(seed=1)[1:],
    'ring with contained reads': _ring_with_contained,
    'linear, several unitigs': lambda: GC.linear(3, n_reads=60)[1:],
    'linear 150': lambda: GC.linear(1)[1:],
    'no reads': lambda: ([], []),
}


def _layout(G, reads, slack, drift):
    cstart, tasks, arena = G.consensus_layout(reads, GC.COMPLEMENT, slack=slack, drift=drift)
    return cstart.tolist(), tasks.tolist(), arena.read(0, arena.nbytes), arena.nbytes


@pytest.mark.parametrize('name', sorted(CASES))
def test_placements_tasks_and_arena_equal_the_oracle(name):
    from biseqt_amd.graph import PLACE_DTYPE, TASK_DTYPE, OverlapGraph
    reads, records = CASES[name]()
    lens = [len(r) for r in reads]
    built = GR.build(lens, records)
    places = CR.place(lens, records, built)
    draft = GR.contigs(reads, built['unitigs'], built['members'], GC.COMPLEMENT)
    with OverlapGraph(lens) as G:
        if records:
            G.add(records)
        G.build()
        assert GC.snapshot(G) == built
        got = G.placements()
        assert got.dtype == PLACE_DTYPE and got.tolist() == places
        before = G.device_bytes
        for slack, drift in CC.PARAMS:
            want_tasks, want_cstart, want_bytes = CR.tasks(lens, places, built['unitigs'], slack, drift)
            cstart, tasks, arena, nbytes = _layout(G, reads, slack, drift)
            assert cstart == want_cstart and tasks == want_tasks and nbytes == want_bytes
            assert (arena == CR.arena(reads, draft, want_tasks, want_cstart, want_bytes, GC.COMPLEMENT)).all()
            assert int(G.lib.pw_graph_cons_num_cols(G.handle)) == want_cstart[-1]
            assert G.lib.pw_graph_cons_tasks_device(G.handle) and G.lib.pw_graph_cons_cstart_device(G.handle)
            # every frame is where a batch may read it
            assert all(t[0] % 4 == 0 and t[1] % 16 == 0 and -lens[t[2]] <= t[4] <= t[5] <= t[3] for t in tasks)
        assert G.device_bytes >= before + want_bytes
        assert G.placements().tolist() == places and G.consensus_layout(reads, GC.COMPLEMENT)[2].nbytes > 0
        assert np.zeros(1, TASK_DTYPE).itemsize == 40


def test_accessors_before_their_stage_and_after_a_rebuild():
    from biseqt_amd import _pwlib as W
    from biseqt_amd.graph import OverlapGraph
    _, reads, records, _ = CC.chains()
    lens = [len(r) for r in reads]
    out = np.zeros(8 * len(lens) + 64, np.int64)
    with OverlapGraph(lens) as G:
        lib, h = G.lib, G.handle
        G.add(records)

        def nothing_laid_out(why):
            for f in ('pw_graph_cons_num_tasks', 'pw_graph_cons_num_cols', 'pw_graph_cons_arena_bytes'):
                assert getattr(lib, f)(h) == -1 and why in W.last_error()
            for f in ('pw_graph_cons_cstart', 'pw_graph_cons_tasks'):
                assert getattr(lib, f)(h, out.ctypes.data) == -1 and why in W.last_error()
            for f in ('pw_graph_cons_cstart_device', 'pw_graph_cons_tasks_device', 'pw_graph_cons_arena_device'):
                assert not getattr(lib, f)(h)

        def nothing_placed():
            assert lib.pw_graph_placements(h, out.ctypes.data) == -1 and 'before pw_graph_place' in W.last_error()
            assert not lib.pw_graph_placements_device(h)

        assert lib.pw_graph_place(h, None) == -1 and 'before pw_graph_build' in W.last_error()
        with pytest.raises(RuntimeError, match='before pw_graph_build'):
            G.placements()
        with pytest.raises(RuntimeError, match='before pw_graph_build'):
            G.consensus_layout(reads, GC.COMPLEMENT)
        nothing_placed(); nothing_laid_out('before pw_graph_consensus_layout')
        G.build()
        nothing_placed(); nothing_laid_out('before pw_graph_consensus_layout')
        first = G.placements()
        assert lib.pw_graph_placements_device(h)
        nothing_laid_out('before pw_graph_consensus_layout')            # placed, not laid out
        for bad in (dict(slack=-1), dict(drift=-.5), dict(drift=float('nan')), dict(drift=float('inf'))):
            with pytest.raises(ValueError):
                G.consensus_layout(reads, GC.COMPLEMENT, **bad)
        comp = np.ascontiguousarray(GC.COMPLEMENT)
        offs = np.zeros(len(lens), np.int64)
        assert lib.pw_graph_consensus_layout(h, None, offs.ctypes.data, comp.ctypes.data, 4, -1, .1, None) == -1 and 'slack' in W.last_error()
        assert lib.pw_graph_consensus_layout(h, None, offs.ctypes.data, comp.ctypes.data, 4, 5, -1., None) == -1 and 'drift' in W.last_error()
        with pytest.raises(ValueError, match='complement'):
            G.consensus_layout(reads)                                    # reverse-complemented reads and no table
        cstart, tasks, arena = G.consensus_layout(reads, GC.COMPLEMENT)
        assert len(tasks) == len(lens) and arena.nbytes == int(lib.pw_graph_cons_arena_bytes(h))
        arena.close()                                                    # an adopted arena frees nothing
        assert G.consensus_layout(reads, GC.COMPLEMENT)[1].tolist() == tasks.tolist()
        G.contigs(reads, GC.COMPLEMENT)                                  # new contig letters drop the layout, not the placements
        nothing_laid_out('before pw_graph_consensus_layout')
        assert lib.pw_graph_placements_device(h)
        G.consensus_layout(reads, GC.COMPLEMENT)
        G.build(min_overlap=10 ** 6)                                     # every overlap is weak now: a rebuild drops everything
        nothing_placed(); nothing_laid_out('before pw_graph_consensus_layout')
        again = G.placements()
        assert again.tolist() == [(u, 0, 0, u, 0) for u in range(len(lens))] and again.tolist() != first.tolist()
        assert len(G.consensus_layout(reads, GC.COMPLEMENT)[1]) == len(lens)


def test_adopt_wraps_without_owning():
    from biseqt_amd.batch import DeviceArena
    host = np.arange(64, dtype=np.uint8)
    with DeviceArena(host) as dev:
        view = DeviceArena.adopt(dev.ptr + 16, 32, dev.device, owner=dev)
        assert view.read().tolist() == host[16:48].tolist() and view.read(4, 3).tolist() == [20, 21, 22]
        view.close(); view.close()
        assert view.ptr is None and dev.read(0, 4).tolist() == [0, 1, 2, 3]          # the owner's memory is still there
        with pytest.raises(ValueError):
            DeviceArena.adopt(0, 16)
