"""The cases of tests/stream_cases.py discriminate: from the oracle alone (no GPU), every pair of the probe batch has
another answer in every two of its arenas -- score, end cell, start or transcript -- and the packed offsets differ from pair
1 on, so a stale read shows in every field tests/test_gpu_streams.py compares.  The arenas share one geometry."""
import itertools

import numpy as np
import pytest

from tests import stream_cases as SC


def test_arenas_share_one_geometry_and_the_batch_layout():
    geo = SC.geometry(**SC.PROBE)
    assert len(geo) == 64 and all(60 <= x <= 300 and 52 <= y <= x for x, y in geo)
    layouts = []
    for a in range(SC.ARENAS):
        pairs = SC.probe_pairs(a)
        assert [(len(o), len(m)) for o, m in pairs] == geo
        none = [k for k, (o, m) in enumerate(pairs) if not set(o.tolist()) & set(m.tolist())]
        assert none == list(range(7 - a, 64, 8)), (a, none)          # every eighth pair has no letter in common
        arena, offs = SC.layout(pairs)
        layouts.append(offs)
        assert all(oo % 16 == 0 and mo % 16 == 0 for oo, mo in offs)
    assert layouts[0] == layouts[1] == layouts[2]
    assert not np.array_equal(SC.layout(SC.probe_pairs(0))[0], SC.layout(SC.probe_pairs(1))[0])


@pytest.mark.parametrize('name', sorted(SC.TYPES))
def test_every_pair_and_every_packed_offset_differs_between_arenas(oracle, name):
    exp = [SC.expected(oracle, a, name) for a in range(SC.ARENAS)]
    for e in exp:
        assert sum(1 for t in e.txs if t) >= 48, name
        assert int(e.packed_offsets[-1]) == len(e.packed_bytes) == sum(len(t or '') for t in e.txs)
    for a, b in itertools.combinations(range(SC.ARENAS), 2):
        same = [k for k in range(64) if exp[a].view[k] == exp[b].view[k]]
        assert not same, (name, a, b, same)
        eq = np.flatnonzero(exp[a].packed_offsets[1:] == exp[b].packed_offsets[1:]) + 1
        assert eq.size == 0, (name, a, b, eq.tolist())
        # ... and so do what the references make of the transcripts, as wholes
        assert exp[a].summaries != exp[b].summaries
        for form in ('extended', 'classic'):
            assert exp[a].cigars[form][1].tolist() != exp[b].cigars[form][1].tolist()
        n_cols = len(SC.layout(exp[a].pairs)[0])
        assert (exp[a].pileup(n_cols) != exp[b].pileup(n_cols)).any()


def test_family_cases_differ_between_poison_and_probe(oracle):
    """The larger cases of the kernel-family test (two arenas each): every pair differs."""
    for fam, (name, case, band, no_common) in SC.FAMILY_CASES.items():
        if fam == 'strip':                   # (36e6 cells in the oracle: the GPU test asserts the difference itself)
            continue
        y, x = (SC.expected(oracle, a, name, case, band, no_common) for a in (0, 1))
        assert all(v[3] for v in y.view) and all(v[3] for v in x.view), name
        assert [k for k in range(case['n']) if y.view[k] == x.view[k]] == [], name
        assert (y.packed_offsets[1:] != x.packed_offsets[1:]).all(), name
