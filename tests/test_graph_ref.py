"""The CPU oracle of the overlap graph (tests/graph_ref.py) against what the contract promises, without a GPU: error-free
linear layouts on both strands give one unitig that spells the genome, a ring gives one circular unitig that is a rotation
of it, a hand-computed case of five reads has every array written out, and kept arcs come in twin pairs.  Also the
ctypes side of include/pw_graph.h: exports, constants and record sizes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import graph_cases as GC
from tests import graph_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kept(arcs):
    return [a for a in arcs if not a[5] & R.REMOVED]


@pytest.mark.parametrize('seed', [1, 2, 3])
@pytest.mark.parametrize('fuzz', [0, 10])
def test_error_free_linear_layout_is_one_unitig_that_spells_the_genome(seed, fuzz):
    genome, reads, recs = GC.linear(seed)
    assert len(reads) == 150 and all(300 <= len(r) <= 500 for r in reads) and {r[2] for r in recs} == {0, 1}
    out = R.build([len(r) for r in reads], recs, fuzz=fuzz)
    (unitig,) = out['unitigs']
    assert unitig[1] == 6000 and unitig[4] == 0 and unitig[2] == 150 - sum(out['contained']) == len(out['members'])
    (letters,) = R.contigs(reads, out['unitigs'], out['members'], GC.COMPLEMENT)
    assert bytes(bytearray(letters)) in (genome.tobytes(), GC.rc(genome).tobytes())
    # a reduced layout: every member keeps one arc to each side but the two ends
    assert len(_kept(out['arcs'])) == 2 * (unitig[2] - 1) < len(out['arcs'])


def test_thin_coverage_gives_several_unitigs_that_are_pieces_of_the_genome():
    genome, reads, recs = GC.linear(3, n_reads=60)
    out = R.build([len(r) for r in reads], recs)
    assert len(out['unitigs']) == 3
    for letters in R.contigs(reads, out['unitigs'], out['members'], GC.COMPLEMENT):
        assert bytes(bytearray(letters)) in genome.tobytes() or bytes(bytearray(letters)) in GC.rc(genome).tobytes()


@pytest.mark.parametrize('n', [12, 65])
def test_ring_is_one_circular_unitig_that_is_a_rotation_of_the_genome(n):
    genome, reads, recs = GC.ring(n)
    out = R.build([len(r) for r in reads], recs)
    assert len(out['arcs']) == 6 * n and len(_kept(out['arcs'])) == 2 * n and sum(out['contained']) == 0
    assert out['unitigs'] == [(0, 100 * n, n, 0, 1)]
    assert [m[1] for m in out['members']] == [100] * n and out['members'][0][0] == 0
    (letters,) = R.contigs(reads, out['unitigs'], out['members'], GC.COMPLEMENT)
    assert GC.is_rotation(letters, genome) or GC.is_rotation(letters, GC.rc(genome))


def test_hand_computed_case_of_five_reads():
    """Reads of 100 letters at 0, 40 and 80 of a genome of 220 (reads 0, 1, 2, forwards), read 3 the letters 50 .. 90 (inside
    read 1), read 4 the letters 120 .. 220 stored reverse-complemented.  0 -> 2 -> 4 -> 9 spells the genome; 0 -> 4 is the
    transitive arc (40 + 40 <= 80 + fuzz); the chain 8 -> 5 -> 3 -> 1 is the dropped twin."""
    rng = np.random.RandomState(11)
    genome = rng.randint(0, 4, 220).astype(np.uint8)
    reads = [genome[0:100], genome[40:140], genome[80:180], genome[50:90], GC.rc(genome[120:220])]
    lens = [100, 100, 100, 40, 100]
    recs = [(0, 1, 0, 40, 100, 0, 60, 60, 60), (0, 2, 0, 80, 100, 0, 20, 20, 20), (1, 2, 0, 40, 100, 0, 60, 60, 60),
            (1, 3, 0, 10, 50, 0, 40, 40, 40), (2, 4, 1, 40, 100, 0, 60, 60, 60), (3, 4, 0, 0, 0, 0, 0, 0, 0)]
    out = R.build(lens, recs, fuzz=10)
    assert out['cls'] == [R.A_TO_B, R.A_TO_B, R.A_TO_B, R.B_CONTAINED, R.A_TO_B, R.NONE]
    assert out['contained'] == [0, 0, 0, 1, 0]
    assert out['arcs'] == [(0, 2, 40, 60, 0, 4), (0, 4, 80, 20, 1, 3), (2, 4, 40, 60, 2, 4), (3, 1, 40, 60, 0, 4), (4, 9, 40, 60, 4, 4),
                           (5, 3, 40, 60, 2, 4), (5, 1, 80, 20, 1, 3), (8, 5, 40, 60, 4, 4)]
    assert out['rows'] == [0, 2, 2, 3, 4, 5, 7, 7, 7, 8, 8]
    assert out['unitigs'] == [(0, 220, 4, 0, 0)]
    assert out['members'] == [(0, 40, 0), (2, 40, 40), (4, 40, 80), (9, 100, 120)]
    assert R.contigs(reads, out['unitigs'], out['members'], GC.COMPLEMENT) == [genome.tolist()]
    # without the fuzz the arc is still transitive (80 <= 80); one letter less on it and it is not
    assert R.build(lens, recs, fuzz=0)['arcs'] == out['arcs']
    recs[1] = (0, 2, 0, 79, 100, 0, 21, 21, 21)
    assert [a[5] for a in R.build(lens, recs, fuzz=0)['arcs'] if a[4] == 1] == [0, 0]


@pytest.mark.parametrize('case', ['linear', 'thin', 'ring', 'ladder'])
def test_every_kept_arc_s_twin_is_kept(case):
    _, reads, recs = dict(linear=lambda: GC.linear(2), thin=lambda: GC.linear(1, n_reads=60), ring=lambda: GC.ring(12),
                          ladder=lambda: GC.ladder(40, 400, 20, both_strands=True))[case]()
    arcs = R.build([len(r) for r in reads], recs)['arcs']
    kept = {(a[0], a[1], a[4]) for a in _kept(arcs)}
    assert kept and all((w ^ 1, v ^ 1, src) in kept for v, w, src in kept)
    assert all(bool(a[5] & R.CHAIN) <= (not a[5] & R.REMOVED) for a in arcs)


def test_duplicate_keys_are_refused():
    with pytest.raises(ValueError, match='duplicate'):
        R.build([100, 100], [(0, 1, 0, 60, 100, 0, 40, 40, 40)] * 2)


def test_exports_constants_and_records_match_the_header():
    from biseqt_amd import _pwlib as W
    from biseqt_amd import graph as G
    txt = open(os.path.join(ROOT, 'include', 'pw_graph.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    declared = set(re.findall(r'\b(pw_\w+)\s*\(', txt))
    assert declared == set(W.GRAPH_EXPORTS), declared ^ set(W.GRAPH_EXPORTS)
    lib = W.load()
    for name in declared:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    enum = re.search(r'enum \{([^}]*)\}', txt).group(1)
    for name, value in re.findall(r'(PW_OVL_\w+) = (\d+)', enum):
        assert getattr(W, name) == int(value) == getattr(R, name[7:]) == getattr(G, name[7:]), name
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define\s+(PW_ARC_\w+)\s+(\d+)\b', txt)}
    assert defines == dict(PW_ARC_REDUCED=R.REDUCED, PW_ARC_REMOVED=R.REMOVED, PW_ARC_CHAIN=R.CHAIN)
    assert all(getattr(W, k) == v for k, v in defines.items())
    W.check_layout()
    for struct, dtype in ((W.pw_graph_overlap, G.OVERLAP_DTYPE), (W.pw_graph_arc, G.ARC_DTYPE), (W.pw_unitig, G.UNITIG_DTYPE),
                          (W.pw_unitig_member, G.MEMBER_DTYPE)):
        assert C.sizeof(struct) == dtype.itemsize
        assert [(n, getattr(struct, n).offset) for n, _ in struct._fields_] == [(n, dtype.fields[n][1]) for n in dtype.names]


def test_argument_errors_before_any_device_work():
    from biseqt_amd.graph import OverlapGraph
    with pytest.raises(ValueError):
        OverlapGraph([100, -1])
