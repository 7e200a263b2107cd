"""The consensus stage without a GPU: the oracle of tests/consensus_ref.py (include/pw_consensus.h restated) pinned to letters
on error-free reads, and the whole consensus on the oracle side on noisy reads, so that the fixture is known to meet the
conditions the GPU tests rely on.

The experiment as run here (tests/consensus_cases.py: a 2000-letter genome, 125 reads of 400 letters on both strands -- 25x --
with 3 % substitutions, 2 % insertions, 2 % deletions, 2126 true overlaps of at least 150 letters aligned by the CPU oracle,
B_OVERLAP 1 / -3 / -5 / -2 in a band of +-40; layout with slack 50, drift .1; two insertion slots, min_depth 3, self weight
1): one contig of 1996 letters from 121 member reads (reads of one length are rarely contained: 4 are), all 125 reads
placed, 125 tasks, all aligned; error total of the draft against the genome 136, of the polished contig 14."""
import numpy as np
import pytest

from tests import consensus_cases as CC
from tests import consensus_ref as CR
from tests import graph_cases as GC
from tests import graph_ref as GR


def _check_letters(reads, records, circular=False):
    lens = [len(r) for r in reads]
    built = GR.build(lens, records)
    draft = GR.contigs(reads, built['unitigs'], built['members'], GC.COMPLEMENT)
    places = CR.place(lens, records, built)
    assert all(p[0] >= 0 for p in places)
    for r, (u, rev, pos, root, depth) in enumerate(places):
        assert (depth == 0) == (not built['contained'][r]) and (depth > 0 or root == r) and not built['contained'][root]
        o = CR.oriented(reads[r], rev, GC.COMPLEMENT)
        lo, hi = max(pos, 0), min(pos + lens[r], len(draft[u]))
        assert lo < hi or circular, (r, pos)
        assert (o[lo - pos:hi - pos] == np.array(draft[u][lo:hi], np.uint8)).all(), (r, places[r])
        if not circular:                                      # a linear contig of error-free reads holds every read whole
            assert 0 <= pos and pos + lens[r] <= len(draft[u])
    return built, places


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_error_free_linear_reads_lie_where_they_are_placed(seed):
    _, reads, records = GC.linear(seed, both_strands=True)
    built, places = _check_letters(reads, records)
    assert sum(built['contained']) > 10 and any(p[1] for p in places) and any(not p[1] for p in places)


def test_error_free_ring_reads_lie_where_they_are_placed():
    for seed in (1, 2):
        _, reads, records = GC.ring(seed=seed)
        built, places = _check_letters(reads, records, circular=True)
        assert [u[4] for u in built['unitigs']] == [1]
    # contained reads on a ring: a read of half the length inside every second read
    genome, reads, records = GC.ring(seed=3)
    n = len(reads)
    for r in range(0, n, 2):
        reads.append(reads[r][100:300].copy())
        records.append((r, n + r // 2, 0, 100, 300, 0, 200, 200, 200))
    _check_letters(reads, sorted(records), circular=True)


def test_chains_pin_the_table_and_the_composition():
    genome, reads, records, spans = CC.chains()
    lens = [len(r) for r in reads]
    built, places = _check_letters(reads, records)
    assert sorted(p[4] for p in places if p[4]) == sorted(d for n in CC.CHAIN_LINKS for d in range(1, n + 1))
    # every row of the table was used by a winning parent record, and both branches of the composition
    links = CR.parent_links(lens, [tuple(r) for r in records], built['cls'])
    rows = set()
    for c, (p, rel, off) in links.items():
        rec = next(r for r in records if (r[0], r[1]) in ((c, p), (p, c)))
        rows.add((built['cls'][records.index(rec)], rec[2]))
    assert rows == {(3, 0), (3, 1), (4, 0), (4, 1)}
    assert {places[p][1] for _, (p, _, _) in links.items()} == {0, 1}
    assert any(v & 1 for v, _, _ in built['members']) and {p[2] % 4 for p in places} == {0, 1, 2, 3}
    # the contig is the genome (or its reverse complement), so every read lies where it was cut from
    (u,) = built['unitigs']
    draft = np.array(GR.contigs(reads, built['unitigs'], built['members'], GC.COMPLEMENT)[0], np.uint8)
    flipped = not (draft == genome).all()
    assert (draft == (GC.rc(genome) if flipped else genome)).all()
    for r, (s, e, o) in enumerate(spans):
        assert places[r][1] == o ^ flipped and places[r][2] == (len(genome) - e if flipped else s)


def test_planted_cases_by_the_oracle():
    cases = CC.planted()
    reads, records = cases['tie']
    lens = [len(r) for r in reads]
    built = GR.build(lens, records)
    assert built['contained'] == [0, 0, 0, 1, 1]
    places = CR.place(lens, records, built)
    assert places[3][3:] == (0, 1) and places[4][3:] == (1, 1)
    reads, records = cases['cycles']
    lens = [len(r) for r in reads]
    places = CR.place(lens, records, GR.build(lens, records))
    assert places[3:] == [CR.UNPLACED] * 6 and all(p[0] == 0 for p in places[:3])
    reads, records = cases['edges']
    lens = [len(r) for r in reads]
    built = GR.build(lens, records)
    assert built['contained'] == [0, 0, 0] + [1] * 4 + [0] + [1] * 5
    places = CR.place(lens, records, built)
    assert all(p[0] >= 0 for p in places)
    length = built['unitigs'][0][1]
    tasks, cstart, _ = CR.tasks(lens, places, built['unitigs'], 50, .1)
    with_task = {t[2] for t in tasks}
    assert any(p[2] < 0 and r in with_task for r, p in enumerate(places)), places
    assert any(p[0] == 0 and p[2] + lens[r] > length and r in with_task for r, p in enumerate(places)), places
    assert any(p[0] == 0 and lens[r] and (p[2] + lens[r] <= 0 or p[2] >= length) for r, p in enumerate(places)), places
    assert 7 not in with_task and 12 not in with_task and len(built['unitigs']) == 2 and built['unitigs'][1][1] == 0
    # windows are clipped at both ends of the contig, and not everywhere
    assert any(t[0] == 0 for t in tasks) and any(t[0] + t[3] == length for t in tasks)
    tight, _, _ = CR.tasks(lens, places, built['unitigs'], 0, 0.)
    assert [t[2] for t in tight] == [t[2] for t in tasks] and all(t[3] <= lens[t[2]] + 3 for t in tight)
    reads, records = cases['no_arcs']
    lens = [len(r) for r in reads]
    built = GR.build(lens, records)
    places = CR.place(lens, records, built)
    assert places == [(u, 0, 0, u, 0) for u in range(4)]
    tasks, cstart, arena_bytes = CR.tasks(lens, places, built['unitigs'], 50, .1)
    assert cstart == [0, 40, 40, 104, 112] and [t[2] for t in tasks] == [0, 2, 3]
    assert [t[1] for t in tasks] == [112, 176, 256] and arena_bytes == 256 + 32 + 16
    arena = CR.arena(reads, [r for r in reads], tasks, cstart, arena_bytes)
    assert (arena[37:40] == 255).all() and (arena[109:112] == 255).all() and (arena[104:109] == reads[3]).all()
    assert (arena[176:240] == reads[2]).all() and not arena[240:256].any() and (arena[256:261] == reads[3]).all()


def test_whole_consensus_on_the_oracle_side(oracle):
    """The fixture's conditions: a contig of at least half the genome, a draft that is at least 40 errors from the genome, and
    a polished total of less than half the draft's -- the floor DESIGN.md K16 uses for read correction: a rule that does
    nothing misses it.  (The module docstring has the figures.)"""
    nf = CC.noisy_fixture()
    fx, genome = nf['fx'], nf['genome']
    assert '-' in fx['strands'] and '+' in fx['strands']
    got = CC.oracle_consensus(oracle, fx['reads'], CC.oracle_records(oracle))
    lengths = [u[1] for u in got['built']['unitigs']]
    placed = sum(p[0] >= 0 for p in got['places'])
    before, after = CC.errors(got['draft'], genome), CC.errors(got['contigs'], genome)
    print('pairs %d, contigs %r, members %d, placed %d of %d, tasks %d, aligned %d; errors: draft %d, polished %d'
          % (len(fx['pairs']), lengths, len(got['built']['members']), placed, len(fx['reads']), len(got['tasks']), got['aligned'],
             before, after))
    assert max(lengths) >= len(genome) // 2
    assert before >= 40
    assert 2 * after < before, (before, after)
    assert sum(got['built']['contained']) >= 1 and any(p[1] for p in got['places']) and any(not p[1] for p in got['places'])


def test_exports_and_records_match_the_header():
    import ctypes as C
    import os
    import re
    from biseqt_amd import _pwlib as W
    from biseqt_amd import graph as G
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, 'include', 'pw_consensus.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    declared = set(re.findall(r'\b(pw_\w+)\s*\(', txt))
    assert declared == set(W.CONSENSUS_EXPORTS), declared ^ set(W.CONSENSUS_EXPORTS)
    lib = W.load()
    for name in declared:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    W.check_layout()
    for struct, dtype in ((W.pw_cons_place, G.PLACE_DTYPE), (W.pw_cons_task, G.TASK_DTYPE)):
        assert C.sizeof(struct) == dtype.itemsize == W.SIZEOF[struct.__name__]
        assert [(n, getattr(struct, n).offset) for n, _ in struct._fields_] == [(n, dtype.fields[n][1]) for n in dtype.names]
