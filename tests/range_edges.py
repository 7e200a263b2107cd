"""The planner's range bounds at their edges: one table shared by tests/test_range_edges.py (the CPU lane emulator) and
tests/test_gpu_range_edges.py (the GPU).

Every kernel choice of the planner rests on a range bound proved by hand in a comment (biseqt_amd/csrc/pw_plan.h,
admit_packed and packed_matrix_bytes_ok; pwlib_api.cpp, batch_plan).  Each row below names one bound and gives, for every
alignment rule and kernel layout the bound covers, an INSIDE case -- the guarded quantity at its limit -- and an OUTSIDE
case one unit past it, with the kernel the planner must report for each and pairs that actually reach the quantity.  The
numbers are computed here from the bound's own formula (`quantity`), not written down by hand, and every case checks that
its quantity is on the side it claims.

A case is a dict: ``id``, ``bound`` (the formula and its source), ``side``, ``quantity`` / ``limit``, ``pairs`` (distinct
pairs), ``copies`` (each pair is repeated that often in the batch), ``kw`` (the oracle's / emulator's scoring arguments),
``env`` (``PWLIB_*`` knobs for the planner), ``expect`` (what ``batch.plan_only`` must report: a dict of its fields plus
``kernel_has`` / ``kernel_lacks`` substrings; ``strips='all'``: every pair on the strips), ``reference`` (the flag of the GPU run the whole batch is compared with) and
``gpu_only`` (a reason, where the emulator cannot run the case in the suite's time)."""
import numpy as np

from biseqt_amd import _pwlib as W

# alignment types by packed rule (pw_plan.h, packed_rule): (name, mode, alntype)
B_LOCAL, LOCAL, END_ANCHORED = ('B_LOCAL', 1, 1), ('LOCAL', 0, 1), ('END_ANCHORED', 0, 3)
START_ANCHORED, B_OVERLAP, B_GLOBAL, GLOBAL = ('START_ANCHORED', 0, 2), ('B_OVERLAP', 1, 2), ('B_GLOBAL', 1, 0), ('GLOBAL', 0, 0)
RULE = {'B_LOCAL': 0, 'LOCAL': 0, 'END_ANCHORED': 4, 'START_ANCHORED': 5, 'B_OVERLAP': 1, 'B_GLOBAL': 2, 'GLOBAL': 2}

# packed layouts (pw_plan.h, packed_lane_layout / packed_workgroup_layout) and the knobs that give them: one pair per
# wavefront at the narrowest lanes, several pairs side by side, a workgroup of wavefronts per pair (latency mode, a band
# that needs 16+ diagonals per lane on one wavefront)
LAYOUTS = ('wave', 'lanes', 'workgroup')


def _layout_env(layout, ndiag):
    """Knobs for a layout.  One pair per wavefront is what the planner gives bands too wide for two pairs side by side at
    the narrowest lanes (ndiag > 32 x 4: the cases use such bands); lane packing is forced at the narrowest lanes that
    leave room for two pairs; workgroups come with latency mode and bands that need 16+ diagonals per lane."""
    if layout == 'workgroup':
        assert ndiag > 64 * 12, ndiag
        return {'PWLIB_LATENCY_MODE': '1'}
    if layout == 'lanes':
        bk = next(b for b in (4, 8, 12, 16, 20, 24, 28, 32) if 32 * b >= ndiag)
        return {'PWLIB_LATENCY_MODE': '0', 'PWLIB_PACKED_BK': '%ds' % bk}
    assert 32 * 4 < ndiag <= 64 * 4, ndiag
    return {'PWLIB_LATENCY_MODE': '0'}


def _layout_marks(layout):
    return {'wave': dict(kernel_has=['false'], kernel_lacks=['_mw']), 'lanes': dict(kernel_has=['true']),
            'workgroup': dict(kernel_has=['k_fill16_mw'])}[layout]


def _ndiag(mode, X, Y, band):
    return X + Y + 1 if mode == 0 else min(band[1], X) - max(band[0], -Y) + 1


def identical(n, L=4, seed=0):
    o = np.random.default_rng(seed).integers(0, L, n).astype(np.uint8)
    return o, o.copy()


def unrelated(n, Y=None):
    """One letter against another: every substitution a mismatch."""
    return np.zeros(n, np.uint8), np.ones(n if Y is None else Y, np.uint8)


def mutated(n, L=4, seed=1, rate=0.05, dels=()):
    rng = np.random.default_rng(seed)
    o = rng.integers(0, L, n).astype(np.uint8)
    m = o.copy()
    hit = rng.random(n) < rate
    m[hit] = (m[hit] + 1 + rng.integers(0, L - 1, int(hit.sum()))) % L
    keep = np.ones(n, bool)
    for a, b in dels:
        keep[a:b] = False
    return o, m[keep]


def gap_heavy(n, L=4, seed=2, run=6, every=25):
    """Runs of `run` deletions every `every` letters (the mutant) and the same letters inserted (the origin is longer)."""
    o = np.random.default_rng(seed).integers(0, L, n).astype(np.uint8)
    keep = np.ones(n, bool)
    for a in range(every // 2, n - run, every):
        keep[a:a + run] = False
    return o, o[keep]


def _case(cases, rid, bound, side, quantity, limit, pairs, kw, expect, copies=1, env=None, reference=W.PW_FLAG_NO_PACKED16,
          gpu_only=None, label=''):
    inside = side == 'inside'
    assert (quantity <= limit) == inside, (rid, side, quantity, limit)
    cases.append(dict(id='%s-%s%s' % (rid, side, '-' + label if label else ''), row=rid, bound=bound, side=side,
                      quantity=quantity, limit=limit, pairs=pairs, copies=copies, kw=kw, env=dict(env or {}),
                      expect=expect, reference=reference, gpu_only=gpu_only))


def _packed_expect(rule, layout, x4=False, matrix=None):
    e = dict(packed_rule=3 if (rule == 0 and x4) else rule, score_dtype='i32', **_layout_marks(layout))
    if matrix is not None:
        e['matrix'] = matrix
    return e


NOT_PACKED = dict(packed_rule=-1, score_dtype='i32')


def best(maxmin, smax):
    """No cell scores above min(X, Y) best substitutions (admit_packed: `best`)."""
    return maxmin * max(0, smax)


def lowest(maxmin, smin, go, ge, maxnd):
    """The lowest in-band score of rules 1, 2, 5 (admit_packed: `lowest`)."""
    return maxmin * max(0, -smin) + abs(go) + abs(ge) * (maxnd + 2)


def _kw(t, L=4, band=None, **sc):
    kw = dict(mode=t[1], alntype=t[2], L=L, **sc)
    if t[1] == 1:
        kw['diag_range'] = band
    return kw


def cases():
    out = []
    # ---- rules 0 / 4: best <= 8000 (pw_plan.h admit_packed, `if (rule == 0 || rule == 4) fits = best <= 8000`) ----
    bound = 'rules 0 / 4: best = min(X, Y) * max(0, smax) <= 8000 (pw_plan.h, admit_packed)'
    sc = dict(match=100., mismatch=-100., go=-50., ge=-50.)
    for t, bands in ((B_LOCAL, [((-80, 80), 'wave'), ((-21, 21), 'lanes'), ((1, 21), 'lanes'), ((-21, -1), 'lanes')]),
                     (LOCAL, [(None, 'wave'), (None, 'lanes')]), (END_ANCHORED, [(None, 'wave'), (None, 'lanes')])):
        for band, layout in bands:
            for side, n in (('inside', 80), ('outside', 81)):
                kw = _kw(t, band=band, **sc)
                nd = _ndiag(t[1], n, n, band or (0, 0))
                exp = _packed_expect(RULE[t[0]], layout) if side == 'inside' else NOT_PACKED
                _case(out, 'best8000', bound, side, best(n, 100), 8000, [identical(n), mutated(n, dels=[(30, 33)])], kw,
                      exp, copies=300, env=_layout_env(layout, nd), label='%s%s-%s' % (t[0], band or '', layout))
    # ... with match 1 over a long pair, the band one diagonal off the true alignment (the leak of
    # test_band_edge_never_leaks_long_pairs, there at 9000 only); the workgroup on a wide band
    sc = dict(match=1., mismatch=-1., go=-1., ge=-1.)
    for band, layout in (((1, 21), 'lanes'), ((-21, -1), 'lanes'), ((1, 1100), 'workgroup')):
        for side, n in (('inside', 8000), ('outside', 8001)):
            kw = _kw(B_LOCAL, band=band, **sc)
            exp = _packed_expect(0, layout) if side == 'inside' else dict(packed_rule=-1)
            _case(out, 'best8000long', bound, side, best(n, 1), 8000, [identical(n, seed=3)], kw, exp,
                  copies=300 if layout != 'workgroup' else 4, env=_layout_env(layout, _ndiag(1, n, n, band)),
                  label='%s-%s' % (band, layout),
                  gpu_only='8000 x 8000 on an 1100-diagonal band: minutes in the emulator' if layout == 'workgroup' else None)
    # ---- rule 5: best <= 8000 and lowest <= 23000 ----
    bound = 'rule 5: best <= 8000 and lowest = min(X, Y) * max(0, -smin) + |go| + |ge| (maxnd + 2) <= 23000 (admit_packed)'
    for layout in ('wave', 'lanes'):
        sc = dict(match=100., mismatch=-100., go=-50., ge=-50.)             # the best term binds
        for side, n in (('inside', 80), ('outside', 81)):
            assert lowest(n, -100, -50, -50, 2 * n + 1) <= 23000
            exp = _packed_expect(5, layout) if side == 'inside' else NOT_PACKED
            _case(out, 'rule5best', bound, side, best(n, 100), 8000, [identical(n), unrelated(n)],
                  _kw(START_ANCHORED, **sc), exp, copies=300, env=_layout_env(layout, 2 * n + 1), label=layout)
        sc = dict(match=1., mismatch=-100., go=-50., ge=-50.)               # the lowest term binds
        for side, n in (('inside', 114), ('outside', 115)):
            q = lowest(n, -100, -50, -50, 2 * n + 1)
            exp = _packed_expect(5, layout) if side == 'inside' else NOT_PACKED
            _case(out, 'rule5lowest', bound, side, q, 23000, [identical(n), unrelated(n)], _kw(START_ANCHORED, **sc), exp,
                  copies=300, env=_layout_env(layout, 2 * n + 1), label=layout)
    # ---- rules 1 / 2: lowest <= 23000, best <= 30000 ----
    bound = 'rules 1 / 2: lowest = min(X, Y) * max(0, -smin) + |go| + |ge| (maxnd + 2) <= 23000 (admit_packed)'
    sc = dict(match=1., mismatch=-100., go=0., ge=-4.)
    for t in (B_GLOBAL, B_OVERLAP):
        for layout, band in (('wave', (-70, 70)), ('lanes', (-10, 10))):
            nd = band[1] - band[0] + 1
            for side in ('inside', 'outside'):
                n = max(k for k in range(1, 2000) if lowest(k, -100, 0, -4, nd) <= 23000) + (side == 'outside')
                q = lowest(n, -100, 0, -4, nd)
                # all mismatches; and an origin longer than its mutant, for the gap run down to the last diagonal
                pairs = [unrelated(n), unrelated(n + band[1], n)]
                exp = _packed_expect(RULE[t[0]], layout) if side == 'inside' else NOT_PACKED
                _case(out, 'lowest23000', bound, side, q, 23000, pairs, _kw(t, band=band, **sc), exp,
                      copies=300, env=_layout_env(layout, nd), label='%s-%s' % (t[0], layout))
    bound = 'rules 1 / 2: best = min(X, Y) * max(0, smax) <= 30000 (admit_packed)'
    sc = dict(match=100., mismatch=-1., go=0., ge=-1.)
    for t in (B_GLOBAL, B_OVERLAP):
        for layout, band in (('wave', (-70, 70)), ('lanes', (-10, 10))):
            for side, n in (('inside', 300), ('outside', 301)):
                nd = band[1] - band[0] + 1
                assert lowest(n, -1, 0, -1, nd) <= 23000
                exp = _packed_expect(RULE[t[0]], layout) if side == 'inside' else NOT_PACKED
                _case(out, 'best30000', bound, side, best(n, 100), 30000, [identical(n)], _kw(t, band=band, **sc), exp,
                      copies=300, env=_layout_env(layout, nd), label='%s-%s' % (t[0], layout))
    # ---- every score within +-100, go <= 0, ge <= 0 ----
    bound = 'max|score| <= 100 (|go + ge| included), go <= 0, ge <= 0 (admit_packed)'
    for t in (B_LOCAL, B_OVERLAP, B_GLOBAL):
        for layout, band in (('wave', (-70, 70)), ('lanes', (-12, 20))):
            nd = band[1] - band[0] + 1
            for side, go, ge in (('inside', -60., -40.), ('outside', -61., -40.)):
                exp = _packed_expect(RULE[t[0]], layout, x4=True) if side == 'inside' else NOT_PACKED
                _case(out, 'maxabs100', bound, side, abs(go + ge), 100, [gap_heavy(200, run=2), mutated(200, dels=[(50, 58)])],
                      _kw(t, band=band, match=1., mismatch=-1., go=go, ge=ge), exp, copies=300,
                      env=_layout_env(layout, nd), label='%s-%s' % (t[0], layout))
            for side, ge in (('inside', 0.), ('outside', 1.)):
                exp = _packed_expect(RULE[t[0]], layout, x4=True) if side == 'inside' else NOT_PACKED
                _case(out, 'ge0', bound, side, ge, 0, [gap_heavy(200, run=2)], _kw(t, band=band, match=1., mismatch=-1., go=-5., ge=ge),
                      exp, copies=300, env=_layout_env(layout, nd), label='%s-%s' % (t[0], layout))
    # ---- X + Y + 2 < 32000: steps counted in signed 16 bits ----
    bound = 'maxspan = X + Y + 2 < 32000 (admit_packed)'
    sc = dict(match=1., mismatch=-1., go=-1., ge=-1.)
    for layout, band, copies in (('lanes', (-5, 5), 300), ('workgroup', (-1100, 1100), 2)):
        for side, X in (('inside', 15998), ('outside', 15999)):
            o, m = mutated(16000, seed=7, dels=[(9000, 9001)])          # mutant 15999 letters
            o = o[:X]
            exp = _packed_expect(2, layout) if side == 'inside' else dict(packed_rule=-1)
            _case(out, 'span32000', bound, side, X + len(m) + 2, 31999, [(o, m)], _kw(B_GLOBAL, band=band, **sc), exp,
                  copies=copies, env=_layout_env(layout, band[1] - band[0] + 1), label=layout,
                  gpu_only='16 k x 16 k on a 2201-diagonal band: minutes in the emulator' if layout == 'workgroup' else None)
    # ---- rule 3 (scores times 4): best <= 2047; its matrix form: 4 (smax - smin) <= 127 ----
    bound = 'rule 3: best <= 2047 (admit_packed, a.x4)'
    sc = dict(match=1., mismatch=-3., go=-5., ge=-2.)
    for layout, band in (('wave', (-100, 100)), ('lanes', (-12, 12)), ('workgroup', (-500, 500))):
        for side, n in (('inside', 2047), ('outside', 2048)):
            exp = _packed_expect(0, layout, x4=side == 'inside')
            _case(out, 'x4best2047', bound, side, best(n, 1), 2047, [identical(n, seed=4), mutated(n, seed=5, dels=[(700, 704)])],
                  _kw(B_LOCAL, band=band, **sc), exp, copies=300 if layout != 'workgroup' else 4,
                  env=_layout_env(layout, band[1] - band[0] + 1), label=layout)
    bound = 'rule 3 matrix form: 4 (smax - smin) <= 127 (pw_plan.h, packed_matrix_bytes_ok(x4))'
    for side, mm in (('inside', -30.), ('outside', -31.)):
        # config 2's layout (one pair per wavefront, 8 diagonals per lane): match / mismatch on the matrix form
        exp = dict(packed_rule=3 if side == 'inside' else 0, matrix=True, kernel_has=['k_fill16<8, false>'])
        _case(out, 'x4matrix31', bound, side, 1 - mm, 31, [identical(600, seed=6), mutated(600, seed=7, rate=0.3)],
              _kw(B_LOCAL, band=(-200, 200), match=1., mismatch=mm, go=-5., ge=-2.), exp, copies=300,
              env={'PWLIB_LATENCY_MODE': '0'})
    # ---- the packed matrix bytes: smax - smin <= 127 and smin <= 0 ----
    bound = 'matrix bytes: smax - smin <= 127, smin <= 0 (pw_plan.h, packed_matrix_bytes_ok)'

    def matrix(lo, hi):
        S = np.full((4, 4), -7.)
        np.fill_diagonal(S, hi)
        S[0, 1], S[2, 3], S[3, 0] = lo, lo, lo + 1
        return S.tolist()
    for t in (B_LOCAL, B_OVERLAP, B_GLOBAL):
        for layout, band in (('wave', (-70, 70)), ('lanes', (-10, 10))):
            nd = band[1] - band[0] + 1
            for side, hi in (('inside', 27.), ('outside', 28.)):
                exp = _packed_expect(RULE[t[0]], layout, matrix=True) if side == 'inside' else NOT_PACKED
                o, m = mutated(150, seed=8, rate=0.4)
                _case(out, 'matrix127', bound, side, hi + 100, 127, [(o, m), identical(150), unrelated(150)],
                      _kw(t, band=band, subst=matrix(-100., hi), go=-5., ge=-2.), exp, copies=300,
                      env=_layout_env(layout, nd), label='%s-%s' % (t[0], layout))
            for side, lo in (('inside', 0.), ('outside', 1.)):
                S = np.full((4, 4), lo + 2)
                np.fill_diagonal(S, 10.)
                S[1, 2] = lo
                exp = _packed_expect(RULE[t[0]], layout, x4=True, matrix=True) if side == 'inside' else NOT_PACKED
                _case(out, 'matrixmin0', bound, side, lo, 0, [mutated(150, seed=9, rate=0.4), unrelated(150)],
                      _kw(t, band=band, subst=S.tolist(), go=-5., ge=-2.), exp, copies=300,
                      env=_layout_env(layout, nd), label='%s-%s' % (t[0], layout))
    # ---- a positive mismatch score forces the matrix form (admit_packed, force_matrix) ----
    bound = 'mismatch > 0: the matrix form, smax - smin <= 127 (admit_packed, force_matrix)'
    for t in (B_LOCAL, B_OVERLAP, B_GLOBAL):
        for side, mm in (('inside', 27.), ('outside', 28.)):
            # a diagonal that waits long for its first cell: origin far longer than its mutant, a band off to one side
            rng = np.random.default_rng(10)
            o, m = rng.integers(0, 4, 60).astype(np.uint8), rng.integers(0, 4, 290).astype(np.uint8)
            band = (-280, -200) if t is not B_GLOBAL else (-280, 0)
            exp = dict(packed_rule=RULE[t[0]], matrix=True) if side == 'inside' else NOT_PACKED
            _case(out, 'posmismatch', bound, side, mm + 100, 127, [(o, m), unrelated(60, 290)],
                  _kw(t, band=band, match=-100., mismatch=mm, go=-3., ge=-1.), exp, copies=300,
                  env={'PWLIB_LATENCY_MODE': '0'}, label=t[0])
    # ---- int32 exact: maxspan * maxabs < 2^27 (pwlib_api.cpp, batch_plan: use_f64) ----
    bound = 'int32: (X + Y + 2) * max|score| < 2^27 (pwlib_api.cpp, batch_plan)'
    span = 602
    for t in (GLOBAL, LOCAL):
        for side in ('inside', 'outside'):
            a = ((1 << 27) - 1) // span + (side == 'outside')          # the largest max|score| with span * a < 2^27, + 1
            sc = dict(match=float(a), mismatch=-float(a), go=-1000., ge=-float(a - 1000))
            exp = dict(score_dtype='i32' if side == 'inside' else 'f64', packed_rule=-1, strips=0)
            _case(out, 'int32', bound, side, span * a, (1 << 27) - 1, [identical(300), unrelated(300), gap_heavy(300, run=15)],
                  _kw(t, **sc), exp, copies=1, reference=W.PW_FLAG_FORCE_F64, label=t[0])
    # ---- the strips: maxspan * maxabs < 2^25 (batch_plan: strips_serve) ----
    bound = 'strips: (X + Y + 2) * max|score| < 2^25 (pwlib_api.cpp, batch_plan: strips_serve)'
    span = 2002
    for t in (LOCAL, GLOBAL):
        for side in ('inside', 'outside'):
            a = ((1 << 25) - 1) // span + (side == 'outside')
            sc = dict(match=float(a), mismatch=-float(a), go=-3., ge=-2.)
            for flags in ((0, W.PW_FLAG_FORCE_STRIP) if side == 'outside' else (0,)):
                exp = dict(strips='all', score_dtype='i32') if side == 'inside' else dict(strips=0, score_dtype='i32')
                _case(out, 'strips2e25', bound, side, span * a, (1 << 25) - 1, [identical(1000, seed=11), unrelated(1000)],
                      _kw(t, **sc), exp, reference=W.PW_FLAG_FORCE_F64, label='%s%s' % (t[0], '-force' if flags else ''))
                out[-1]['flags'] = flags
    # ---- the strips' byte rows: every score an integer in [-128, 127], L <= 4 (pwlib_api.cpp, strip_byte_rows_ok) ----
    bound = 'strip byte rows: integer scores in [-128, 127], L <= 4 (pwlib_api.cpp, strips_serve / strip_byte_rows_ok)'
    for side, lo, hi in (('inside', -128., 127.), ('outside', -129., 127.), ('outside', -128., 128.)):
        S = np.full((4, 4), -3.)
        np.fill_diagonal(S, 5.)
        S[0, 0], S[1, 2], S[2, 1] = hi, lo, lo
        exp = dict(strips='all' if side == 'inside' else 0, score_dtype='i32')
        _case(out, 'striprows', bound, side, max(hi, -lo - 1), 127, [mutated(1000, seed=12, rate=0.3), unrelated(1000)],
              _kw(LOCAL, subst=S.tolist(), go=-3., ge=-2.), exp, reference=W.PW_FLAG_FORCE_F64,
              label='%d..%d' % (lo, hi))
    for side, mt in (('inside', 127.), ('outside', 128.)):
        # match / mismatch: byte rows up to 127, compare and select beyond -- the strips either way
        _case(out, 'striprows-simple', bound, side, mt, 127, [identical(1000, seed=13), mutated(1000, seed=14, rate=0.3)],
              _kw(LOCAL, match=mt, mismatch=-128., go=-3., ge=-2.), dict(strips='all', score_dtype='i32'),
              reference=W.PW_FLAG_FORCE_F64)
    # ---- dyadic scaling: multiples of 2^-k, k <= 10 (pw_plan.h, summarise_scores) ----
    bound = 'dyadic scores: multiples of 2^-k, k <= 10, held times 2^k (summarise_scores); int32 while span * maxabs * 2^k < 2^27'
    for side, k in (('inside', 10), ('outside', 11)):
        sc = dict(match=2. ** -k, mismatch=-1., go=0., ge=-1.)       # config 5's score shape, the match scaled down
        exp = dict(score_dtype='i32', scale_shift=10) if side == 'inside' else dict(score_dtype='f64', scale_shift=0)
        _case(out, 'dyadic', bound, side, k, 10, [mutated(400, seed=15, rate=0.1, dels=[(100, 103)])],
              _kw(B_GLOBAL, band=(-20, 20), **sc), exp, copies=4, reference=W.PW_FLAG_FORCE_F64)
    for side, X in (('inside', 1022), ('outside', 1023)):
        sc = dict(match=2. ** -10, mismatch=-64., go=0., ge=-64.)     # scaled max|score| 2^16: int32 below span 2048
        o, m = mutated(1023, seed=16, rate=0.05)
        o = o[:X]
        exp = dict(score_dtype='i32' if side == 'inside' else 'f64', scale_shift=10)
        _case(out, 'dyadic2e27', bound, side, (X + len(m) + 2) * 64 * 1024, (1 << 27) - 1, [(o, m)],
              _kw(B_GLOBAL, band=(-20, 20), **sc), exp, copies=4, reference=W.PW_FLAG_FORCE_F64)
    return out


def batch_of(case):
    """(pairs, per-pair bands or None) of the batch: every distinct pair `copies` times."""
    return [p for p in case['pairs'] for _ in range(case['copies'])]
