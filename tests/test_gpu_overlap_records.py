"""Every field of the overlap band records (include/pw_overlap.h: pw_overlap_band) against the independent CPU oracle
oracle/overlap_record_oracle.py, on the named cases of tests/overlap_cases.py -- pairs that tests/test_overlap_cases.py proves
(on the CPU) to take each scoring path: one wavefront (<= 64 seeds), one workgroup from the seed list (65 .. 2048 seeds,
all-pairs path), the histogram kernel with <= 1024, <= 8192 and more occupied diagonals, and the reverse-strand encoders
and join.  Every comparison is exact equality, w_best included as a double: the header promises IEEE double in the
reference's operation order.  Records without seeds are compared on n_seeds only (their other fields are undefined)."""
import itertools

import numpy as np
import pytest

from tests import overlap_cases as OC

pytestmark = pytest.mark.gpu

CASES = OC.cases()
GROUPS = OC.groups()
GROUP_IDS = [OC.group_id(key) for key in GROUPS]
E2E_MAX_SEEDS = 5000                                        # the KD-tree oracle keeps one neighbour list per seed
E2E_TOO_DENSE = {'dense_nocc_le_1024', 'dense_nocc_1025_8192', 'dense_nocc_gt_8192', 'w_negative_dense_L2',
                 'clamp_dense_nocc_le_1024', 'clamp_dense_nocc_1025_8192', 'clamp_dense_nocc_gt_8192', 'clamp_short_vs_8300'}   # (asserted below)
E2E_GROUPS = [k for k in GROUPS if not {c.name for c in GROUPS[k]} <= E2E_TOO_DENSE]


def _fields():
    from biseqt_amd.overlap import BAND_DTYPE
    return [name for name in BAND_DTYPE.names if name != 'pad_']


def _diff(rec, o):
    """The fields in which a device record differs from the oracle record: {} when they are equal."""
    if int(rec['n_seeds']) != o['n_seeds']:
        return {'n_seeds': (int(rec['n_seeds']), o['n_seeds'])}
    if o['n_seeds'] == 0:
        return {}
    return {f: (rec[f].item(), o[f]) for f in _fields() if rec[f].item() != o[f]}


def _check(recs, want, names):
    assert len(recs) == len(want)
    bad = {}
    for rec, o, name in zip(recs, want, names):
        d = _diff(rec, o)
        if d:
            bad[name] = d
    assert not bad, bad


def _par(c):
    return c.wordlen, c.alphabet_len, c.g_max, c.sensitivity


def _union(group, minus=False):
    """The distinct reads of a group in interleaved case order (sparse, dense and empty pairs alternate); with `minus`
    every T read is replaced by its reverse complement."""
    reads, seen = [], set()
    for c in OC.interleaved(group):
        S, T = c.reads
        for r in (S, OC.revcomp(T, c.alphabet_len) if minus else T):
            if r.tobytes() not in seen:
                seen.add(r.tobytes())
                reads.append(r)
    return reads


def _expected_all_pairs(reads, c, strands):
    """[(a, b, strand, oracle record)] of every a < b and selected strand with a seed, in ascending (a, b, strand) order."""
    out = []
    for a, b in itertools.combinations(range(len(reads)), 2):
        for st in strands:
            T = OC.revcomp(reads[b], c.alphabet_len) if st else reads[b]
            o = OC.record(reads[a], T, *_par(c))
            if o['n_seeds'] > 0:
                out.append((a, b, st, o))
    return out


# ---- pair-list path ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', CASES, ids=[c.name for c in CASES])
def test_pair_list_one_case(c):
    from biseqt_amd.overlap import raw_bands
    S, T = c.reads
    recs, _ = raw_bands([S, T], [(0, 1)], *_par(c))
    _check(recs, [OC.case_record(c)], [c.name])
    recs, _ = raw_bands([S, T], [(1, 0)], *_par(c))
    _check(recs, [OC.case_record(c, swapped=True)], [c.name + ' swapped'])


@pytest.mark.parametrize('c', CASES, ids=[c.name for c in CASES])
def test_pair_list_one_case_minus_strand(c):
    """T handed over as its reverse complement and scored on the minus strand: the record of the forward pair."""
    from biseqt_amd.overlap import raw_bands
    S, T = c.reads
    rc = lambda x: OC.revcomp(x, c.alphabet_len)
    recs, _ = raw_bands([S, rc(T)], [(0, 1)], *_par(c), strands=['-'], complement=c.complement)
    _check(recs, [OC.case_record(c)], [c.name])
    recs, _ = raw_bands([rc(S), T], [(1, 0)], *_par(c), strands=['-'], complement=c.complement)
    _check(recs, [OC.case_record(c, swapped=True)], [c.name + ' swapped'])


@pytest.mark.parametrize('stranded', [False, True], ids=['forward', 'mixed_strands'])
@pytest.mark.parametrize('key', list(GROUPS), ids=GROUP_IDS)
def test_pair_list_group_in_one_call(key, stranded):
    """All cases of a group in one arena and one call, sparse, dense and empty pairs interleaved (histogram bases and the
    slots of the per-pair seed lists); with `stranded` every other pair goes in as (S, rc(T)) on the minus strand."""
    from biseqt_amd.overlap import raw_bands
    order = OC.interleaved(GROUPS[key])
    reads, pairs, strands = [], [], []
    for q, c in enumerate(order):
        minus = stranded and q % 2 == 0
        reads += [c.reads[0], OC.revcomp(c.reads[1], c.alphabet_len) if minus else c.reads[1]]
        pairs.append((2 * q, 2 * q + 1))
        strands.append('-' if minus else '+')
    kw = dict(strands=strands, complement=order[0].complement) if stranded else {}
    recs, _ = raw_bands(reads, pairs, *_par(order[0]), **kw)
    _check(recs, [OC.case_record(c) for c in order], [c.name for c in order])


# ---- all-pairs path ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('strands', ['+', '-', 'both'])
@pytest.mark.parametrize('key', list(GROUPS), ids=GROUP_IDS)
def test_all_pairs_group(key, strands):
    """The union of a group's reads through one index: exactly the pairs a < b (and strands) with a seed, in ascending
    (a, b, strand) order, every record equal to the oracle's for the materialised pair.  Here the 65 .. 2048-seed pairs are
    scored from the seed list, the larger ones from histogram chunks, with sparse pairs (no histogram) between them."""
    from biseqt_amd.overlap import raw_all_pairs
    c = GROUPS[key][0]
    reads = _union(GROUPS[key], minus=strands != '+')
    sel = {'+': (0,), '-': (1,), 'both': (0, 1)}[strands]
    want = _expected_all_pairs(reads, c, sel)
    if strands == '+':
        pairs, recs, _ = raw_all_pairs(reads, *_par(c))
        flags = np.zeros(len(pairs), np.uint8)
    else:
        pairs, flags, recs, _ = raw_all_pairs(reads, *_par(c), strands=strands, complement=c.complement)
    got = [(int(a), int(b), int(f)) for (a, b), f in zip(pairs.tolist(), flags.tolist())]
    assert got == [(a, b, st) for a, b, st, _ in want]
    _check(recs, [o for _, _, _, o in want], ['(%d, %d, %s)' % (a, b, '+-'[st]) for a, b, st, _ in want])


def test_all_pairs_shards_partition_and_match_the_oracle():
    from biseqt_amd.overlap import raw_all_pairs
    key = max(GROUPS, key=lambda k: len(GROUPS[k]))
    c = GROUPS[key][0]
    reads = _union(GROUPS[key])
    want = {(a, b): o for a, b, _, o in _expected_all_pairs(reads, c, (0,))}
    seen = []
    for rank in range(2):
        pairs, recs, _ = raw_all_pairs(reads, *_par(c), rank=rank, world=2)
        got = [tuple(p) for p in pairs.tolist()]
        assert got == sorted(got) and all(a % 2 == rank for a, _ in got)
        _check(recs, [want[p] for p in got], [str(p) for p in got])
        seen += got
    assert sorted(seen) == sorted(want) and len(set(seen)) == len(seen)
    assert {a % 2 for a, _ in seen} == {0, 1}


# ---- end to end: the reference's dicts ------------------------------------------------------------------------------
def _alphabet(L):
    from biseqt_amd.sequence import Alphabet
    return Alphabet('ACGT' if L == 4 else 'ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789'[:L])


def _same(a, b):
    return len(a) == len(b) and bool((a == b).all())


def test_end_to_end_leaves_out_only_what_the_kdtree_oracle_cannot_hold():
    assert {c.name for c in CASES if OC.case_record(c)['n_seeds'] > E2E_MAX_SEEDS} == E2E_TOO_DENSE


@pytest.mark.parametrize('key', E2E_GROUPS, ids=OC.group_id)
def test_end_to_end_dicts_vs_kdtree_oracle(key):
    """overlap_bands on the cases the KD-tree oracle can hold: the tie > 1 cases take the single-pair fallback, the
    w_best <= 0 cases the first-row branch; the fallback count is the oracle's."""
    from biseqt_amd.overlap import overlap_bands
    from oracle import blot_oracle as BO
    order = [c for c in OC.interleaved(GROUPS[key]) if c.name not in E2E_TOO_DENSE]
    c0 = order[0]
    reads = [r for c in order for r in c.reads]
    pairs = [(2 * q, 2 * q + 1) for q in range(len(order))]
    stats = {}
    got = overlap_bands(reads, pairs, c0.wordlen, _alphabet(c0.alphabet_len), c0.g_max, c0.sensitivity, stats=stats)
    fallback = 0
    for c, g in zip(order, got):
        S, T = c.reads
        assert not _same(S, T)
        o = OC.case_record(c)
        fallback += o['n_seeds'] > 0 and o['w_best'] > 0 and o['tie'] > 1
        e = BO.highest_scoring_overlap_band(S.tolist(), T.tolist(), c.wordlen, c.alphabet_len, c.g_max, c.sensitivity)
        assert g == e, (c.name, g, e)
    assert stats['fallback_pairs'] == fallback


# The KD-tree oracle takes about 0.15 ms per seed of a pair here (one Python neighbour list per seed), so every test below
# compares the pairs of its union in ascending seed count until it has spent E2E_SEED_BUDGET seeds -- about three seconds.
E2E_SEED_BUDGET = 25000


@pytest.mark.parametrize('key', E2E_GROUPS, ids=OC.group_id)
def test_end_to_end_all_pairs_vs_kdtree_oracle(key):
    """overlap_all_pairs over the union of every group's reads (the cases the KD-tree oracle cannot hold left out): the keys
    are the oracle's pairs with a seed, the fallback count is the oracle's count over ALL listed pairs, and the dicts equal
    the KD-tree oracle's on as many pairs, smallest first, as the seed budget allows."""
    from biseqt_amd.overlap import overlap_all_pairs
    from oracle import blot_oracle as BO
    group = [c for c in GROUPS[key] if c.name not in E2E_TOO_DENSE]
    c = group[0]
    reads = _union(group)
    stats = {}
    got = overlap_all_pairs(reads, c.wordlen, _alphabet(c.alphabet_len), c.g_max, c.sensitivity, stats=stats)
    want = _expected_all_pairs(reads, c, (0,))
    assert list(got) == [(a, b) for a, b, _, _ in want]
    differ = [(a, b, o) for a, b, _, o in want if not _same(reads[a], reads[b])]     # (identical reads: the documented divergence)
    assert stats['fallback_pairs'] == sum(o['w_best'] > 0 and o['tie'] > 1 for _, _, o in differ)
    spent = compared = 0
    for a, b, o in sorted(differ, key=lambda t: (t[2]['n_seeds'], t[0], t[1])):
        if o['n_seeds'] > E2E_MAX_SEEDS or spent + o['n_seeds'] > E2E_SEED_BUDGET:
            break
        spent += o['n_seeds']
        e = BO.highest_scoring_overlap_band(reads[a].tolist(), reads[b].tolist(), c.wordlen, c.alphabet_len, c.g_max,
                                            c.sensitivity)
        assert got[(a, b)] == e, (a, b, got[(a, b)], e)
        compared += 1
    assert compared or not differ
