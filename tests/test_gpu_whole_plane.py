"""Whole tie-mask planes, walks from any end cell and score planes on the GPU, against the oracle.

Every kernel family is reached through the product's planner (flags and ``PWLIB_*`` knobs) and its ``kernel_name`` is
asserted, so each case covers what it claims.  Masks: ``BatchAligner.masks(k)`` (``pw_batch_masks``) must equal the
oracle's mask on every in-table cell -- all four bits, except on the packed 16-bit kernels and the strips, which store no
M bit (tests/test_emu_whole_plane.py gives the walker's argument): bits 0-2 there, with go <= 0.  Walks: a batch of copies
of one pair, each copy with its own end cell (every cell of small tables, 2000 of larger ones, a few (-1, -1)), must equal
``pwo_traceback_from``.  Score planes: ``scores_plane`` / ``pw_batch_table`` against the oracle's H."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import dec, kw_of, load_golden
from tests.plane_checks import bkw_of, check_masks, check_walks, okw_of

pytestmark = pytest.mark.gpu

MAX_ENDS = 2000
SC = dict(match=1, mismatch=-3, go=-5, ge=-2)
MAT = [[2, -1, -2, -1], [-1, 3, -1, -2], [-2, -1, 2, -1], [-1, -2, -1, 1]]


def related(n, seed, Y=None):
    from biseqt_amd import synth
    rng = synth.rng_for(seed)
    o = synth.rand_seqs(rng, 1, n)[0]
    m = synth.mutate(rng, o, 0.1, 0.04, 0.4)
    return o, (m if Y is None else m[:Y])


def table_cells(res, X, Y, mode):
    if mode == 0:
        return [(i, j) for i in range(X + 1) for j in range(Y + 1)]
    out = []
    for i in range(res['num_rows']):
        d = res['band'][0] + i
        out += [(i, a) for a in range(1 + min(d, 0) + min(X - d, Y))]
    return out


def pick_ends(cells, seed):
    """Every cell of a small table, else a random sample: 2000 cells, fewer on tables the oracle takes long to walk."""
    rng = np.random.default_rng(seed)
    n = min(MAX_ENDS, int(4e8 // len(cells)))
    ends = list(cells) if len(cells) <= n else [cells[int(k)] for k in rng.choice(len(cells), n, replace=False)]
    for q in range(0, len(ends), 97):
        ends.insert(q, (-1, -1))
    return ends


# (id, kernel substrings, kw, (X, Y), flags name, env): every family of the fill kernels
FAMILIES = [
    ('fill16-wave', ['k_fill16<', 'false>'], dict(mode=1, alntype=1, diag_range=(-100, 100), **SC), (300, 290), 0,
     {'PWLIB_LATENCY_MODE': '0', 'PWLIB_SIMPLE_AS_MATRIX': '0', 'PWLIB_NO_SCALED16': '1'}),
    ('fill16-lanes', ['k_fill16<', 'true>'], dict(mode=1, alntype=1, diag_range=(-60, 60), **SC), (200, 190), 0,
     {'PWLIB_LATENCY_MODE': '0', 'PWLIB_PACKED_BK': '4s', 'PWLIB_SIMPLE_AS_MATRIX': '0', 'PWLIB_NO_SCALED16': '1'}),
    ('fill16-mw', ['k_fill16_mw'], dict(mode=1, alntype=1, diag_range=(-500, 500), **SC), (700, 690), 0,
     {'PWLIB_LATENCY_MODE': '1'}),
    ('fill16-x4', ['x4'], dict(mode=1, alntype=1, diag_range=(-100, 100), **SC), (300, 290), 0,
     {'PWLIB_LATENCY_MODE': '0', 'PWLIB_SIMPLE_AS_MATRIX': '0'}),
    ('fill16-matrix', ['k_fill16<', ', 2> matrix'], dict(mode=1, alntype=0, diag_range=(-100, 100), subst=MAT, go=-5, ge=-2),
     (300, 290), 0, {'PWLIB_LATENCY_MODE': '0'}),
    ('fill16-x4-matrix', ['k_fill16<8, false> x4 matrix'], dict(mode=1, alntype=1, diag_range=(-200, 200), **SC), (400, 390),
     0, {'PWLIB_LATENCY_MODE': '0'}),
    ('fill16-rule4', ['k_fill16<', ', 4>'], dict(mode=0, alntype=3, **SC), (60, 55), 0, {}),
    ('fill16-rule5', ['k_fill16<', ', 5>'], dict(mode=0, alntype=2, **SC), (60, 55), 0, {}),
    ('fill-fast', ['k_fill<int', 'false, false, false>'], dict(mode=1, alntype=0, diag_range=(-40, 40), **SC), (120, 110),
     'NO_PACKED16', {}),
    ('fill-track', ['k_fill<int', 'false, true, false>'], dict(mode=0, alntype=2, **SC), (50, 45), 'NO_PACKED16', {}),
    ('fill-any', ['k_fill<int', 'true, true, false>'], dict(mode=0, alntype=1, **SC), (50, 45), 'NO_PACKED16', {}),
    ('fill-f64', ['k_fill<double'], dict(mode=0, alntype=4, **SC), (50, 45), 'FORCE_F64', {}),
    ('fill-generic', ['false, true, true>'], dict(mode=1, alntype=2, diag_range=(-30, 50), match=2, mismatch=-1, go=1, ge=-2),
     (110, 100), 0, {}),
    ('fill-mw', ['k_fill_mw'], dict(mode=0, alntype=1, **SC), (1100, 1050), 'NO_PACKED16', {'PWLIB_NO_STRIP': '1'}),
    ('fill-tiled', ['k_fill_tile'], dict(mode=0, alntype=0, **SC), (150, 140), 'FORCE_TILED', {}),
]


def _flags(name):
    from biseqt_amd import _pwlib as W
    return getattr(W, 'PW_FLAG_' + name) if name else 0


@pytest.mark.parametrize('fam', FAMILIES, ids=[f[0] for f in FAMILIES])
def test_family_masks_and_walks_from_any_end(fam, oracle, monkeypatch):
    from biseqt_amd.batch import BatchAligner
    fid, names, kw, (X, Y), flags, env = fam
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    o, m = related(X, 40 + len(fid), Y)
    okw = okw_of(kw)
    probe = oracle.solve(o, m, **okw)
    ends = pick_ends(table_cells(probe, len(o), len(m), kw['mode']), len(fid))
    with BatchAligner([(o, m)] * len(ends), flags=_flags(flags), **bkw_of(kw)) as b:
        name = b.kernel_name
        assert all(s in name for s in names), (fid, name)
        no_m = 'k_fill16' in name or 'strip' in name
        b.solve()
        b.traceback()
        b.sync()
        res = b.results()
        assert (res['opt_i'][0], res['opt_j'][0]) == probe['opt'], fid
        for k in (0, len(ends) // 2, len(ends) - 1):
            check_masks(oracle, b, k, o, m, okw, no_m, '%s on %s' % (fid, name))
        b.traceback_from(ends)
        b.sync()
        res = b.results()
        txs = b.transcripts(res)
    check_walks(oracle, o, m, okw, ends, res, txs, '%s on %s' % (fid, name))


def test_strips_forced_masks_and_repeated_walks(oracle, monkeypatch):
    """Small tables forced onto the strip pipeline (layout 1): X = 0, 1, 63 (mod 64) and flat tables, byte rows and a
    matrix; every cell's mask, then traceback_from again and again on one solved batch."""
    monkeypatch.setenv('PWLIB_NO_STRIP_REPAIR', '1')
    from biseqt_amd import _pwlib as W
    from biseqt_amd.batch import BatchAligner
    shapes = [(128, 40), (129, 70), (127, 33), (64, 3), (191, 100)]
    for q, (X, Y) in enumerate(shapes):
        for kw in (dict(mode=0, alntype=q % 7, **SC), dict(mode=0, alntype=(q + 3) % 7, subst=MAT, go=-3, ge=-1)):
            o, m = related(X, 70 + q, Y)
            okw = okw_of(kw)
            with BatchAligner([(o, m), (m[:50], o[:60])], flags=W.PW_FLAG_FORCE_STRIP, **bkw_of(kw)) as b:
                assert 'strip' in b.kernel_name, b.kernel_name
                b.run()
                check_masks(oracle, b, 0, o, m, okw, True, 'strips %dx%d' % (X, Y))
                check_masks(oracle, b, 1, m[:50], o[:60], okw, True, 'strips 50x60')
                probe = oracle.solve(o, m, **okw)
                cells = table_cells(probe, len(o), len(m), 0)
                rng = np.random.default_rng(q)
                for r in range(12):
                    e = cells[int(rng.integers(0, len(cells)))] if r else (0, 0)
                    b.traceback_from([e, (-1, -1)])
                    b.sync()
                    res = b.results()
                    check_walks(oracle, o, m, okw, [e], res[:1], b.transcripts(res)[:1], 'strips %dx%d' % (X, Y))


def test_natural_wide_strip_pair_masks_and_walks(oracle, monkeypatch):
    """A 9 kb x 9 kb pair goes to the strips by itself: its whole plane (8e7 cells) and walks from sampled cells."""
    monkeypatch.setenv('PWLIB_NO_STRIP_REPAIR', '1')
    from biseqt_amd.batch import BatchAligner
    o, m = related(9000, 31)
    kw = dict(mode=0, alntype=1, **SC)
    okw = okw_of(kw)
    with BatchAligner([(o, m)], **bkw_of(kw)) as b:
        assert 'strip' in b.kernel_name, b.kernel_name
        b.run()
        check_masks(oracle, b, 0, o, m, okw, True, 'natural strips')
        rng = np.random.default_rng(9)
        for r in range(6):
            e = (int(rng.integers(0, len(o) + 1)), int(rng.integers(0, len(m) + 1)))
            b.traceback_from([e])
            b.sync()
            res = b.results()
            check_walks(oracle, o, m, okw, [e], res, b.transcripts(res), 'natural strips')


def test_config2_sample_whole_planes(oracle, monkeypatch):
    """64 pairs of the batch bench.py times (same seed as test_config2_ten_thousand_pairs_every_kernel_agrees) on
    k_fill16<8, false> x4 matrix: every cell of every plane (about 8e5 each) equals the oracle's mask (bits 0-2)."""
    from biseqt_amd import synth
    from biseqt_amd.batch import BatchAligner
    monkeypatch.setenv('PWLIB_LATENCY_MODE', '0')
    origins, mutants = synth.pair_batch(2, 10000, 2000)
    pick = np.random.default_rng(2).choice(10000, 64, replace=False)
    pairs = [(origins[k], mutants[k]) for k in pick]
    kw = dict(mode=1, alntype=1, diag_range=(-200, 200), **SC)
    okw = okw_of(kw)
    with BatchAligner(pairs, **bkw_of(kw)) as b:
        assert 'k_fill16<8, false> x4 matrix' in b.kernel_name, b.kernel_name
        b.run()
        for k, (o, m) in enumerate(pairs):
            want = check_masks(oracle, b, k, o, m, okw, True, 'config 2 pair %d' % pick[k])
            assert want['mask'].size > 7e5


def test_out_of_table_end_refused_before_launch():
    from biseqt_amd.batch import BatchAligner
    o, m = related(40, 3, 30)
    with BatchAligner([(o, m), (o, m)], alnmode=1, alntype=1, alphabet_len=4, diag_range=(-5, 5), match_score=1,
                      mismatch_score=-3, go_score=-5, ge_score=-2) as b:
        b.solve()
        b.sync()
        for bad in ([[0, 0], [11, 0]], [[0, 0], [0, 40]], [[-1, 3], [0, 0]]):
            with pytest.raises(RuntimeError, match='outside the table'):
                b.traceback_from(bad)


# ---- score planes: five score types ----
PLANES = [
    ('generic-int32', dict(mode=1, alntype=1, diag_range=(-30, 40), match=2, mismatch=-1, go=-3, ge=-1), (80, 75), 0, 0),
    ('generic-f64', dict(mode=0, alntype=4, match=2, mismatch=-1, go=-3, ge=-1), (60, 50), 'FORCE_F64', 0),
    ('logodds-f64', dict(mode=1, alntype=2, diag_range=(-20, 20), match=1.3862943611198906, mismatch=-2.0794415416798357,
                         go=-2.302585092994046, ge=-0.2231435513142097), (70, 66), 0, 0),
    ('dyadic-int32', dict(mode=0, alntype=1, match=0.75, mismatch=-0.5, go=-1.25, ge=-0.25), (70, 60), 0, 2),
    ('dyadic-f64', dict(mode=0, alntype=0, match=1, mismatch=-1, go=-60000.5, ge=-0.5), (600, 600), 0, 1),
]


@pytest.mark.parametrize('case', PLANES, ids=[p[0] for p in PLANES])
def test_score_plane_equals_oracle(case, oracle):
    """scores_plane (banded and standard) and pw_batch_table against the oracle's H on every in-table cell.  dyadic-f64:
    scale shift 1 and span * maxabs >= 2^27, so the batch runs in f64 on doubled scores (pw_batch_scores used to return
    them doubled)."""
    from biseqt_amd import _pwlib as W
    from biseqt_amd.batch import BatchAligner
    cid, kw, (X, Y), flags, _ = case
    o, m = related(X, 90, Y)
    okw = okw_of(kw)
    want = oracle.solve(o, m, want_table=True, **okw)
    with BatchAligner([(o, m)], flags=_flags(flags) | W.PW_FLAG_DUMP_SCORES, **bkw_of(kw)) as b:
        f64 = cid.endswith('f64')
        assert b.lib.pw_batch_score_type(b.handle) == (1 if f64 else 0), cid
        res = b.run()
        assert float(res['score'][0]) == want['score'], cid
        plane = b.scores_plane(0)
        if kw['mode'] == 0:
            tab = np.zeros((X + 1) * (Y + 1), np.float64)
            assert b.lib.pw_batch_table(b.handle, 0, tab.ctypes.data_as(C.POINTER(C.c_double)), tab.size) == 0
    ok = want['mask'] != 0
    cells = table_cells(want, X, Y, kw['mode'])
    flat = np.array([plane[i, j] if kw['mode'] == 1 else plane[i - j + Y, min(i, j)] for i, j in cells])
    assert np.array_equal(flat[ok], want['H'][ok]), (cid, np.nonzero(flat[ok] != want['H'][ok])[0][:5])
    if kw['mode'] == 0:
        assert np.array_equal(tab[ok], want['H'][ok]), cid


# ---- dptable_traceback(T, end) through the reference's own ABI (oracle/ref_driver.py) ----
def _ref_recs():
    return load_golden('explicit_ends.json.gz')


@pytest.mark.parametrize('table', ['banded', 'std-table', 'std-no-table'])
def test_dptable_traceback_from_explicit_ends_equals_reference(table, monkeypatch):
    """Every recorded end cell of tests/golden/explicit_ends.json.gz through libpwlib's dptable_traceback: transcript,
    start and score hex-exact -- also where no table holds the end cell (banded mode, PWLIB_NO_TABLE=1), where the score is
    built along the walk as the reference builds it."""
    from oracle import ref_driver as RD
    from biseqt_amd import _pwlib as W
    if table == 'std-no-table':
        monkeypatch.setenv('PWLIB_NO_TABLE', '1')
    lib = RD.load(W.PWLIB_SO)
    n = nonopt = 0
    for rec in _ref_recs():
        kw = kw_of(rec)
        if (kw.get('mode', 0) == 1) != (table == 'banded'):
            continue
        o, m = dec(rec['origin']), dec(rec['mutant'])
        for e in rec['ends']:
            if e.get('skipped'):
                continue
            P = RD.Problem(o, m, mode=kw.get('mode', 0), alntype=kw.get('alntype', 0), subst=kw['subst'], L=4,
                           go=kw['go'], ge=kw['ge'], diag_range=kw.get('diag_range'), origin_range=kw.get('origin_range'),
                           mutant_range=kw.get('mutant_range'))
            r = RD.run(lib, P, end=tuple(e['end']))
            where = (rec['origin'], rec['mutant'], rec['kw'], e['end'])
            assert r['tb_null'] == e['null'], where
            if e['null']:
                continue
            assert (r['transcript'], r['origin_idx'], r['mutant_idx']) == (e['transcript'], e['origin_idx'],
                                                                          e['mutant_idx']), where
            assert r['tb_score'].hex() == e['score'], (where, r['tb_score'])
            n += 1
            nonopt += tuple(e['end']) != r['opt']
    assert n >= 150 and nonopt >= 100, (n, nonopt)


def test_dptable_traceback_out_of_range_end_returns_null():
    from oracle import ref_driver as RD
    from biseqt_amd import _pwlib as W
    lib = RD.load(W.PWLIB_SO)
    for mode, dr in ((0, None), (1, (-3, 4))):
        P = RD.Problem([0, 1, 2, 3, 0, 1], [0, 1, 3, 3, 1], mode=mode, alntype=1, match=1, mismatch=-1, go=-1, ge=-1,
                       diag_range=dr)
        T = P.table
        assert lib.dptable_init(C.byref(T)) == 0
        lib.dptable_solve(C.byref(T))
        for e in ((99, 0), (0, 99), (-2, 0)):
            assert not lib.dptable_traceback(C.byref(T), RD.intpair(*e)), (mode, e)
        lib.dptable_free(C.byref(T))
