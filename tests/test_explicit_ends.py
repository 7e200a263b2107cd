"""``dptable_traceback(T, end)`` from explicit end cells (pw.c:116-150): the oracle's ``pwo_traceback_from`` pinned to the
reference, field by field, through tests/golden/explicit_ends.json.gz (recorded from the compiled reference by
tests/golden/make_explicit_ends_golden.py).  Scores compare hex-exact."""
from tests.helpers import dec, kw_of, load_golden

RECS = load_golden('explicit_ends.json.gz')


def test_fixture_covers_what_it_claims():
    types = {(r['kw']['mode'], r['kw']['alntype']) for r in RECS}
    assert len(types) == 10, types
    gos = {float.fromhex(r['kw_hex']['go']) for r in RECS}
    assert any(g < 0 for g in gos) and 0.0 in gos and any(g > 0 for g in gos)
    assert any('origin_range' in r['kw'] for r in RECS)
    bands = [tuple(r['kw']['diag_range']) for r in RECS if r['kw']['mode'] == 1]
    assert any(a == b for a, b in bands)
    ends = [e for r in RECS for e in r['ends']]
    assert len(ends) >= 1000 and any(e.get('null') for e in ends) and any(e.get('skipped') for e in ends)
    assert any(e['end'] == [0, 0] for e in ends)


def test_oracle_traceback_from_equals_reference(oracle):
    n = 0
    for rec in RECS:
        o, m, kw = dec(rec['origin']), dec(rec['mutant']), kw_of(rec)
        for e in rec['ends']:
            got = oracle.traceback_from(o, m, e['end'], **kw)
            where = (rec['origin'], rec['mutant'], rec['kw'], e['end'])
            if e.get('skipped'):
                assert (got['no_choice'] if e['skipped'] == 'no_choice' else got['would_panick']), where
                continue
            assert not got['no_choice'] and not got['would_panick'], where
            assert got['tb_null'] == e['null'], where
            if e['null']:
                continue
            assert got['transcript'] == e['transcript'], where
            assert (got['origin_idx'], got['mutant_idx']) == (e['origin_idx'], e['mutant_idx']), where
            assert got['score'].hex() == e['score'], (where, got['score'].hex())
            assert got['maskrule_ok'], where          # the walkers' mask-only rule reproduces the reference's chain
            n += 1
    assert n >= 700, n
