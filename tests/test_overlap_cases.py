"""Every named case of tests/overlap_cases.py lands in the class of scoring path it is meant for -- asserted on the CPU from
oracle/overlap_record_oracle.py alone.  tests/test_gpu_overlap_records.py runs the same cases on the device: a case that
drifts out of its class fails here, not silently there.  No GPU."""
import pytest

from tests import overlap_cases as OC
from tests import wide_words as WW

CASES = OC.cases()


@pytest.mark.parametrize('c', CASES, ids=[c.name for c in CASES])
def test_case_lands_in_its_class(c):
    OC.check_class(c)


def test_the_required_classes_are_all_there():
    rec = {c.name: OC.case_record(c) for c in CASES}
    by = {c.name: c for c in CASES}
    for L in (4, 20):                                   # exact seed counts on both sides of 64 | 65 and 2048 | 2049
        for target in OC.SEED_TARGETS:
            assert rec['seeds%d_L%d' % (target, L)]['n_seeds'] == target
            assert by['seeds%d_L%d' % (target, L)].alphabet_len == L
    assert by['seeds64_L20'].wordlen == 3 and 20 ** 3 & (20 ** 3 - 1)          # L^k is no power of two
    dense = [o for o in rec.values() if o['n_seeds'] > OC.MEDIUM_MAX]
    assert any(o['nocc'] <= OC.KEEP_MAX for o in dense)
    assert any(OC.KEEP_MAX < o['nocc'] <= OC.LISTED_MAX for o in dense)
    assert any(o['nocc'] > OC.LISTED_MAX for o in dense)
    assert any(OC.SMALL_MAX < o['n_seeds'] <= OC.MEDIUM_MAX and o['nocc'] > OC.KEEP_MAX for o in rec.values())
    tables = {len(c.reads[0]) + len(c.reads[1]) + 1 for c in CASES if rec[c.name]['n_seeds'] > OC.SMALL_MAX}
    assert min(tables) < 256 and 256 in tables and any(t % 256 == 1 for t in tables)
    assert any(len(c.reads[0]) == 0 for c in CASES) and any(0 < len(c.reads[0]) < c.wordlen for c in CASES)
    assert any(len(c.reads[0]) == c.wordlen for c in CASES)
    assert any((len(c.reads[0]), len(c.reads[1])) == (30, 3000) for c in CASES)
    assert any(o['n_seeds'] and o['w_best'] == 0 and o['nocc'] > 1 for o in rec.values())
    assert any(o['n_seeds'] and o['w_best'] < 0 and o['nocc'] > 1 for o in rec.values())
    assert any(o['n_seeds'] and o['w_best'] >= 1 for o in rec.values())
    assert any(o['n_seeds'] and 0 < o['w_best'] < 1 and o['tie'] >= 2 for o in rec.values())
    o = rec['near_tie']                                 # a tie that only the rule's tolerance makes: the second score is not the best one
    assert o['tie'] == 2 and OC.tier(o) == 'small' and (o['w'] == o['w_best']).sum() == 1
    # in every tier some occupied diagonal's window crosses the low edge of the table and some the high edge
    for t in ('small', 'medium', 'dense_kept', 'dense_listed', 'dense_chunks'):
        got = [OC.clamped(rec[c.name], *c.reads) for c in CASES if rec[c.name]['n_seeds'] and OC.tier(rec[c.name]) == t]
        assert (True, True) in got, t
    assert {c.g_max for c in CASES} == {.1, .2, .3} and {c.sensitivity for c in CASES} == {.9, .99}
    assert {c.alphabet_len for c in CASES} == {2, 3, 4, 20, 36}
    for L in (3, 36):
        comp = OC.COMPLEMENT[L]
        assert len(comp) == L and (comp[comp] == range(L)).all() and (comp != range(L)).any()
    assert (OC.COMPLEMENT[36][32:] < 4).all()           # letters past 31 go through the complement table
    fixed = [x for x in range(20) if OC.COMPLEMENT[20][x] == x]
    assert len(fixed) == 2 and OC.COMPLEMENT[4].tolist() == [3, 2, 1, 0] and OC.COMPLEMENT[2].tolist() == [1, 0]
    # long words: a group per key width, each with the five classes; the key width cuts the one-call test of the 60-bit group
    # into three chunks (the last one shorter) and that of the 61-bit group into one chunk per pair
    wide = {key[:2]: group for key, group in OC.groups().items() if group[0].name.startswith('wide_')}
    assert set(wide) == set(WW.OVERLAP_RUNGS) and all(len(g) >= 5 for g in wide.values())
    assert sorted((L ** k - 1).bit_length() for L, k in wide) == [32, 32, 57, 60, 61]
    assert (3 ** 20 < 0xffffffff <= 4 ** 16) and 4 ** 16 == 2 ** 32        # the last 4-byte and the first 8-byte key
    for (L, k), group in wide.items():
        tiers = {OC.tier(rec[c.name]) for c in group if rec[c.name]['n_seeds']}
        assert tiers == {'small', 'medium', 'dense_kept'} and any(rec[c.name]['n_seeds'] == 0 for c in group)
        assert any(rec[c.name]['tie'] == 2 and 0 < rec[c.name]['w_best'] < 1 for c in group)
    def chunks(L, k):
        per, n = 2 ** (62 - (L ** k - 1).bit_length()) - 1, len(wide[(L, k)])          # fewer than 2^(62 - kbits) pairs per chunk
        return [min(max(per, 1), n - p0) for p0 in range(0, n, max(per, 1))]
    assert chunks(4, 30) == [3, 3, 1] == WW.chunk_sizes(len(wide[(4, 30)]), 4, 30)
    assert chunks(20, 14) == [1] * len(wide[(20, 14)]) and len(wide[(20, 14)]) >= 5
    assert chunks(36, 11) == [len(wide[(36, 11)])] and chunks(4, 16) == [len(wide[(4, 16)])]
    # every group's call interleaves sparse and dense pairs
    for key, group in OC.groups().items():
        assert sorted(c.name for c in OC.interleaved(group)) == sorted(c.name for c in group)
