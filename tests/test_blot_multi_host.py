"""Multiple-sequence Word-Blot without a GPU: the C ABI of include/pw_mseeds.h is exported, the coordinate maps and the
python-2 pins hold against the reference's fixtures (tests/golden/blot_multi.json.gz), the in-memory class refuses
what the reference refuses, and the CPU yardstick tests/mseeds_ref.py reproduces every fixture."""
import gzip
import json
import math
import os
import re

import numpy as np
import pytest

from biseqt_amd import _pwlib as W
from biseqt_amd.blot import WordBlotMultiple, WordBlotMultipleFast, _check_ref_memory
from biseqt_amd.seeds import SeedIndexMultiple
from biseqt_amd.sequence import Alphabet
from tests import mseeds_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = Alphabet('ACGT')


def golden():
    with gzip.open(os.path.join(ROOT, 'tests', 'golden', 'blot_multi.json.gz'), 'rt') as f:
        return json.load(f)


G = golden()


def test_header_declares_exactly_the_exports_and_the_library_has_them():
    txt = open(os.path.join(ROOT, 'include', 'pw_mseeds.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    declared = set(re.findall(r'\b(pw_mseeds_\w+)\s*\(', txt))
    assert declared == set(W.MSEED_EXPORTS), declared ^ set(W.MSEED_EXPORTS)
    lib = W.load()
    for name in declared:
        assert hasattr(lib, name), name


def test_to_diagonal_and_back():
    rng = np.random.default_rng(3)
    for _ in range(200):
        N = int(rng.integers(2, 9))
        idxs = [int(v) for v in rng.integers(0, 5000, N)]
        ds, a = SeedIndexMultiple.to_diagonal_coordinates(*idxs)
        assert a == sum(idxs) and list(ds) == [idxs[0] - i for i in idxs[1:]]
        assert SeedIndexMultiple.to_ij_coordinates(ds, a) == tuple(idxs)


def test_to_ij_coordinates_uses_python2_floor_division():
    # (a + sum d) = 7 over N = 3: python 2 gives 2, not 2.33
    assert SeedIndexMultiple.to_ij_coordinates((1, -1), 7) == (2, 1, 3)
    assert SeedIndexMultiple.to_ij_coordinates((-4, 0), 2) == (-1, 3, -1)     # floors towards -inf, as python 2 does


def test_to_ij_coordinates_seg_against_the_reference():
    recs = G['to_ij_coordinates_seg']
    assert any(not r['py2_safe'] for r in recs) and any(r['py2_safe'] for r in recs)
    for r in recs:
        ds, a = r['segment']
        got = SeedIndexMultiple.to_ij_coordinates_seg(([tuple(d) for d in ds], tuple(a)))
        # python 2's value is the floor of the python-3 run's (floor is monotone: it commutes with min, max and the clip)
        want = [(math.floor(lo), math.floor(hi)) for lo, hi in r['ij']]
        assert [tuple(x) for x in got] == want, r


def test_check_ref_memory_uses_24_bytes_per_kmer():
    for w in (3, 6, 8, 10):
        need = 24. * 4 ** w / 2 ** 30
        with pytest.raises(MemoryError):
            _check_ref_memory(A, w, need * (1 - 1e-6))
        _check_ref_memory(A, w, need * (1 + 1e-6))
    with pytest.raises(AssertionError):
        _check_ref_memory(A, 4, 0)


def test_memory_refusal_matches_the_reference():
    seqs = [A.parse('ACGTACGTAC'), A.parse('CGTACGTACG')]
    for r in G['memory']:
        allowed = float.fromhex(r['allowed_memory'])
        if r['raises']:
            with pytest.raises(MemoryError):
                WordBlotMultipleFast(*seqs, wordlen=r['wordlen'], alphabet=A, g_max=.2, sensitivity=.9,
                                     allowed_memory=allowed)
        else:
            _check_ref_memory(A, r['wordlen'], allowed)     # (constructing would need a GPU)


def test_argument_refusals():
    S = A.parse('ACGTACGTAC')
    with pytest.raises(AssertionError):
        SeedIndexMultiple(S, S, wordlen=3, alphabet=A)                        # seeds.py:243: more than two
    with pytest.raises(AssertionError):
        WordBlotMultiple(S, S, wordlen=3, alphabet=A, g_max=.2, sensitivity=.9)
    with pytest.raises(AssertionError):
        WordBlotMultipleFast(*([S] * 17), wordlen=3, alphabet=A, g_max=.2, sensitivity=.9)
    with pytest.raises(AssertionError):
        SeedIndexMultiple(S, S, Alphabet('ACGU').parse('ACGU'), wordlen=3, alphabet=A)
    with pytest.raises(AssertionError):
        WordBlotMultipleFast(S, S, S, wordlen=3, alphabet=A, g_max=1.5, sensitivity=.9)


def test_abi_refusals_need_no_device():
    import ctypes as C
    lib = W.load()
    buf = (C.c_uint8 * 4)(0, 1, 2, 3)
    ptrs = (C.c_void_p * 17)(*([C.cast(buf, C.c_void_p).value] * 17))
    lens = (C.c_int64 * 17)(*([4] * 17))
    assert not lib.pw_mseeds_create(0, ptrs, lens, 17, 4, 3)
    assert b'n_seqs' in lib.pw_mseeds_last_error()
    assert not lib.pw_mseeds_create(0, ptrs, lens, 1, 4, 3)
    assert not lib.pw_mseeds_create(0, ptrs, lens, 3, 3, 3)                 # letter 3 outside a 3-letter alphabet
    assert b'alphabet' in lib.pw_mseeds_last_error()
    assert not lib.pw_mseeds_create(0, ptrs, lens, 3, 4, 32)
    big = (C.c_int64 * 3)(1 << 30, 1 << 30, 4)
    assert not lib.pw_mseeds_create(0, ptrs, big, 3, 4, 3)
    assert b'2^31' in lib.pw_mseeds_last_error()


def _seqs(rec):
    return [[ 'ACGT'.index(c) for c in s] for s in rec['seqs']]


@pytest.mark.parametrize('ci', range(len(G['cases'])))
def test_yardstick_reproduces_the_golden(ci):
    rec = G['cases'][ci]
    seqs = _seqs(rec)
    N = len(seqs)
    rows = R.seed_rows(seqs, rec['wordlen'], 4)
    assert rows.tolist() == rec['rows']
    for c in rec['counts']:
        assert R.box_count(rows, c['ds_band'], c['a_band']) == c['count']
    sc = rec['score_seeds']
    if not len(rows):
        assert sc['records'] == []
        return
    g_max, sens = float.fromhex(rec['g_max']), float.fromhex(rec['sensitivity'])
    from biseqt_amd.blot import band_radius
    K = sc['K']
    d_radius = int(np.ceil(band_radius(K, g_max, sens)))
    a_radius = int(np.ceil(N * K / 2.))
    neighs = R.neighbours(rows, d_radius, a_radius)
    assert [r['neighs'] for r in sc['records']] == neighs
    # the components of the segments: every segment's first seed is its component's label
    p = np.array([float.fromhex(r['p']) for r in sc['records']])
    p_min = float.fromhex(rec['similar_segments']['p_min'])
    if rec['similar_segments']['K_min'] == K:
        labels = R.components(neighs, list(p >= p_min))
        assert len(set(x for x in labels if x >= 0)) == len(rec['similar_segments']['plain'])
