"""Whole tie-mask planes and walks from every cell on the CPU lane emulator (tests/emu), against the oracle.

The fill kernels' main output is the tie-mask plane: one nibble per cell with the choices the reference keeps (B 1, D 2,
I 4, M 8).  Elsewhere the suite sees it only along the path the walker takes from the optimal cell.  Here every emulated
kernel form is read back whole through the product's own decoder (pw_strip.h, mask_table) and compared with the oracle's
mask on EVERY in-table cell, and the same plane is walked from every cell (``dptable_traceback(T, end)`` takes any end
cell, pw.c:116-150) and compared with ``pwo_traceback_from`` -- transcript, start and status bits.

Mask rule: kernels that store M match all four bits.  Two families document that they store no M bit: the packed 16-bit
kernels (pw_wave.h, WaveFill16: the nibble is nB + 2 nD + 4 nI) and the strips (pw_strip.h, "the M bit stays 0").  The
walker's predecessor rule (pw_wave.h, trace_walk) reads M only as "the first kept op" when B, D and I are all clear, and
after a gap op with go <= 0 as "the op that led here is not kept, take the first kept one" -- M again exactly when bits
0-2 are clear -- so with go <= 0 the plane without M walks the same.  For those families bits 0-2 are compared exactly and
the batch must have go <= 0 (the planner admits them only then).  No other exemption and no tolerance.

Cells that hold no choice (num_choices == 0; the reference dereferences NULL when a walk starts there) are not walked;
each test reports how many it skipped through its assertion message and checks that the mask there is 0.
"""
import numpy as np
import pytest

from tests import range_edges as R
from tests.emu import emu

WALK_ALL_CELLS = 80 * 80      # tables up to this size are walked from every cell
STRIP_WALKS = 8               # strip walks run on 64 emulated lanes each: a sample per table


def table_cells(res, X, Y, mode):
    """Table coordinates of every in-table cell, in the oracle's mask order."""
    if mode == 0:
        return [(i, j) for i in range(X + 1) for j in range(Y + 1)]
    cells = []
    for i in range(res['num_rows']):
        d = res['band'][0] + i
        cells += [(i, a) for a in range(1 + min(d, 0) + min(X - d, Y))]
    return cells


def pick_ends(cells, limit, seed):
    """Every cell if there are few, else the corners and edges of the table order plus a random sample."""
    if len(cells) <= limit:
        return list(cells)
    rng = np.random.default_rng(seed)
    idx = set([0, len(cells) - 1]) | set(rng.choice(len(cells), limit - 2, replace=False).tolist())
    return [cells[k] for k in sorted(idx)]


_WALKS = {}


def oracle_walk(oracle, o, m, kw, end):
    """``pwo_traceback_from``, kept per problem and end cell: every form walks the same cells of the same tables."""
    key = (np.asarray(o).tobytes(), np.asarray(m).tobytes(), repr(sorted(kw.items())), tuple(end))
    if key not in _WALKS:
        _WALKS[key] = oracle.traceback_from(o, m, end, **kw)
    return _WALKS[key]


def check_plane(oracle, o, m, kw, got, ends, no_m, label):
    """`got`: an emulator result with ``mask`` and ``walks`` for `ends`."""
    X, Y = len(o), len(m)
    want = oracle.solve(o, m, want_table=True, **kw)
    assert got['init_rc'] == want['init_rc'] == 0, label
    assert got['opt'] == want['opt'], label
    bits = 7 if no_m else 15
    if no_m:
        assert kw.get('go', 0.) <= 0, (label, 'a kernel without M bits needs go <= 0')
    wm, gm = want['mask'], got['mask']
    assert gm.shape == wm.shape, label
    bad = np.nonzero((gm & bits) != (wm & bits))[0]
    cells = table_cells(want, X, Y, kw.get('mode', 0))
    assert bad.size == 0, (label, '%d of %d cells differ' % (bad.size, wm.size),
                           [(cells[k], int(wm[k]), int(gm[k])) for k in bad[:8]])
    skipped = 0
    for e, w in zip(ends, got['walks']):
        r = oracle_walk(oracle, o, m, kw, e)
        if r['no_choice']:
            skipped += 1
            continue
        st = w['status']
        assert st & 1 and not st & 8, (label, e, st)
        g = (w['transcript'], (w['origin_idx'], w['mutant_idx']), bool(st & 4), bool(st & 2) and not st & 4)
        x = (r['ops'], r['start'], r['would_panick'], r['tb_null'])
        assert g == x, (label, 'end', e, g, x)
    assert skipped < len(ends) or not ends, (label, 'every end cell held no choice')
    return skipped


def seqs(X, Y, seed, L=4, related=True):
    rng = np.random.default_rng(seed)
    o = rng.integers(0, L, X)
    if related:
        m = o[:Y].copy() if Y <= X else np.concatenate([o, rng.integers(0, L, Y - X)])
        flip = rng.random(Y) < 0.2
        m[flip] = rng.integers(0, L, int(flip.sum()))
    else:
        m = rng.integers(0, L, Y)
    return o, m


def run_form(oracle, o, m, kw, ekw, no_m, label, seed=0, strip=False):
    X, Y = len(o), len(m)
    probe = oracle.solve(o, m, **kw)
    if probe['init_rc'] != 0:           # (a global alignment whose band misses an end point: nothing to fill)
        assert emu.solve(o, m, **dict(kw, **ekw))['init_rc'] == probe['init_rc'], label
        return 0
    cells = table_cells(probe, X, Y, kw.get('mode', 0))
    ends = pick_ends(cells, STRIP_WALKS if strip else WALK_ALL_CELLS, seed)
    if strip:
        got = emu.solve_strip(o, m, want_masks=True, ends=ends, **dict(kw, **ekw))
    else:
        got = emu.solve(o, m, want_masks=True, ends=ends, **dict(kw, **ekw))
    return check_plane(oracle, o, m, kw, got, ends, no_m, label)


# ---- shapes where kernels go wrong: (id, X, Y, mode, band) ----
STD_SHAPES = [('40x33', 40, 33), ('5x70', 5, 70), ('70x5', 70, 5), ('1x30', 1, 30), ('30x1', 30, 1),
              ('32x17', 32, 17), ('47x48', 47, 48), ('31x33', 31, 33), ('16x1', 16, 1)]
BAND_SHAPES = [('40x33b-17..15', 40, 33, (-17, 15)), ('50x50b3..3', 50, 50, (3, 3)), ('45x47b-4..-3', 45, 47, (-4, -3)),
               ('60x30b20..28', 60, 30, (20, 28)), ('30x62b-31..-17', 30, 62, (-31, -17)), ('33x64b-64..1', 33, 64, (-64, 1)),
               ('48x48b-1..0', 48, 48, (-1, 0))]
SCORES = {'plain': dict(match=2, mismatch=-1, go=-3, ge=-1), 'go0': dict(match=1, mismatch=-1, go=0, ge=-1),
          'gopos': dict(match=2, mismatch=-2, go=1, ge=-2), 'negmatch': dict(match=-1, mismatch=-3, go=-2, ge=-2),
          'mm>m': dict(match=-1, mismatch=1, go=-2, ge=-1)}
STD_TYPES = range(7)
BAND_TYPES = range(3)


def _std_cases():
    out = []
    for k, (sid, X, Y) in enumerate(STD_SHAPES):
        for t in STD_TYPES:
            sc = list(SCORES)[(k + t) % len(SCORES)]
            out.append(('std-t%d-%s-%s' % (t, sid, sc), X, Y, dict(mode=0, alntype=t, L=4, **SCORES[sc])))
    for k, (sid, X, Y, band) in enumerate(BAND_SHAPES):
        for t in BAND_TYPES:
            sc = list(SCORES)[(k + t) % len(SCORES)]
            out.append(('band-t%d-%s-%s' % (t, sid, sc), X, Y, dict(mode=1, alntype=t, L=4, diag_range=band, **SCORES[sc])))
    return out


CASES = _std_cases()


@pytest.mark.parametrize('form', ['i32-bk2', 'i32-bk4', 'i32-bk8', 'i32-bk16', 'i32-bk32', 'f64-bk8', 'generic-i32-bk8',
                                  'generic-f64-bk4', 'mw2-i32-bk2', 'mw8-i32-bk2'])
def test_wavefront_kernels_whole_plane(form, oracle):
    """32-bit, f64 and generic wavefront kernels (all four bits), one and several wavefronts per pair, every alignment type
    on every shape."""
    bk = int(form.split('bk')[1])
    ekw = dict(bk=bk, use_double='f64' in form, force_generic='generic' in form,
               waves=int(form[2]) if form.startswith('mw') else 1)
    skipped = 0
    for k, (cid, X, Y, kw) in enumerate(CASES):
        o, m = seqs(X, Y, k)
        nd = X + Y + 1 if kw['mode'] == 0 else 0
        if nd > 64 * ekw['waves'] * bk:
            continue                    # (the table does not fit the form: covered by the wider ones)
        skipped += run_form(oracle, o, m, kw, ekw, False, '%s %s' % (form, cid), seed=k)
    assert skipped == 0


PACKED_FORMS = ['packed-wave', 'packed-lanes', 'packed-x4-wave', 'packed-x4-lanes', 'packed-matrix-wave',
                'packed-matrix-lanes', 'packed-x4-matrix-wave', 'packed-mw2', 'packed-mw4-matrix']


@pytest.mark.parametrize('form', PACKED_FORMS)
def test_packed_kernels_whole_plane(form, oracle):
    """The packed 16-bit body: one pair per wavefront, lane-packed (``nl`` < 64), scores times 4, byte-row matrix, several
    wavefronts per pair; rules 0 .. 5 through the alignment types.  No M bit (module docstring): bits 0-2, go <= 0."""
    lanes = 'lanes' in form
    x4 = 'x4' in form
    mat = 'matrix' in form
    waves = int(form.split('mw')[1][0]) if 'mw' in form else 1
    mode16 = (4 if x4 else 1) if lanes else (3 if x4 else 2)
    rules = set()
    n = 0
    for k, (cid, X, Y, kw) in enumerate(CASES):
        if kw['go'] > 0 or kw['mismatch'] > 0:
            continue                    # (not admitted to the packed kernels: the generic / matrix forms take them)
        rule = R.RULE.get({(0, 0): 'GLOBAL', (0, 1): 'LOCAL', (0, 2): 'START_ANCHORED', (0, 3): 'END_ANCHORED',
                           (1, 0): 'B_GLOBAL', (1, 1): 'B_LOCAL', (1, 2): 'B_OVERLAP'}.get((kw['mode'], kw['alntype'])), -1)
        if rule < 0 or (mat and rule > 2) or (x4 and rule != 0):
            continue                    # (no packed kernel for this type / no matrix form of it / scores times 4: rule 0 only)
        nd = X + Y + 1 if kw['mode'] == 0 else min(kw['diag_range'][1], X) - max(kw['diag_range'][0], -Y) + 1
        bk = 8 if not lanes else next(b for b in (4, 8, 12, 16, 20) if 64 * b >= nd and (nd + b - 1) // b < 64)
        if nd > 64 * waves * bk:
            continue
        o, m = seqs(X, Y, k)
        ekw = dict(bk=bk, packed16=mode16, waves=waves, matrix=mat)
        run_form(oracle, o, m, kw, ekw, True, '%s %s bk%d' % (form, cid, bk), seed=k)
        rules.add(3 if rule == 0 and x4 else rule)
        n += 1
    assert n >= (5 if x4 else 10), n
    assert rules == ({3} if x4 else {0, 1, 2} if mat else {0, 1, 2, 4, 5}), rules


@pytest.mark.parametrize('form', ['strip-byte-rows', 'strip-no-byte-rows', 'strip-matrix'])
def test_strip_whole_plane(form, oracle):
    """The strip pipeline (layout 1): rows X = 0, 1, 63 (mod 64) and tall / flat tables, every standard type; no M bit."""
    mat = [[2, -1, -2, -1], [-1, 3, -1, -2], [-2, -1, 2, -1], [-1, -2, -1, 1]]
    shapes = [(64, 20), (65, 30), (63, 40), (127, 9), (3, 70), (128, 1), (1, 64)]
    for k, (X, Y) in enumerate(shapes):
        for t in STD_TYPES:
            o, m = seqs(X, Y, 100 + k)
            sc = dict(match=2, mismatch=-1, go=-3, ge=-1) if t % 2 else dict(match=1, mismatch=-2, go=0, ge=-2)
            kw = dict(mode=0, alntype=t, L=4, **sc)
            ekw = dict(byte_rows=form != 'strip-no-byte-rows')
            if form == 'strip-matrix':
                kw = dict(mode=0, alntype=t, L=4, subst=mat, go=sc['go'], ge=sc['ge'])
                ekw['subst'] = mat
            run_form(oracle, o, m, kw, ekw, True, '%s %dx%d t%d' % (form, X, Y, t), seed=k * 7 + t, strip=True)


def test_dyadic_scores_whole_plane(oracle):
    """Dyadic scores on the planner's kernels (held times 2^k): the plane must be the oracle's on the unscaled scores."""
    o, m = seqs(60, 57, 5)
    kw = dict(mode=1, alntype=1, L=4, match=0.75, mismatch=-0.5, go=-1.25, ge=-0.25, diag_range=(-20, 9))
    probe = oracle.solve(o, m, **kw)
    ends = pick_ends(table_cells(probe, 60, 57, 1), WALK_ALL_CELLS, 3)
    plan, (got,) = emu.solve_planned([(o, m)], want_masks=True, ends=ends, **kw)
    assert plan['scale_shift'] == 2 and plan['score_dtype'] == 'i32', plan
    check_plane(oracle, o, m, kw, got, ends, plan['packed_rule'] >= 0, 'dyadic on %s' % plan['kernel'])


INSIDE = [c for c in R.cases() if c['side'] == 'inside' and not c['gpu_only']]


@pytest.mark.parametrize('case', INSIDE, ids=[c['id'] for c in INSIDE])
def test_range_edge_inside_whole_plane(case, monkeypatch, oracle):
    """The inside case of every bound of tests/range_edges.py on the kernel the planner picks: every cell's mask, and walks
    from a sample of cells."""
    for k, v in case['env'].items():
        monkeypatch.setenv(k, v)
    kw = case['kw']
    o, m = case['pairs'][0]
    probe = oracle.solve(o, m, **kw)
    strips = R.batch_of(case) and case['expect'].get('strips')
    ends = pick_ends(table_cells(probe, len(o), len(m), kw['mode']), 6 if strips else 64, 11)
    plan, got = emu.solve_planned(R.batch_of(case), flags=case.get('flags', 0), want_masks=True, ends=ends, **kw)
    no_m = plan['packed_rule'] >= 0 or bool(plan['strips'])
    check_plane(oracle, o, m, kw, got[0], ends, no_m, '%s on %s' % (case['id'], plan['kernel']))
