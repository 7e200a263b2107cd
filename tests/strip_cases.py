"""Named inputs for the strip pipeline (K2c: pw_strip.h, pw_strip.hip, launch_strip_fills), each from a fixed RNG seed and
each built to land on one edge of that code: a block kind of ``StripFill::run``, a run boundary of the placement
(``PWLIB_STRIP_RUN``), a wavefront's second strip, a stale granule of an earlier solve, the walker's four-strip window, a
segment cut of the fix-up.  tests/test_strip_cases.py proves from arithmetic and the oracle that every case lands where it
is meant to (and runs some on the lane emulator); tests/test_gpu_strip_edges.py runs the same inputs on the device with the
repair of an abandoned pipeline switched off.

A case is a dict: ``id``, ``family`` (1 .. 6), ``pairs`` (list of (origin, mutant), uint8 letter indices: one batch),
``alntype`` (0 .. 6, standard mode), ``score`` (an entry of tests/micro/strip_check.py's SCORES, or ``MAT``: a 4 x 4
signed-byte matrix with go, ge), ``run_len`` (None: the default placement), ``masks`` (compare the whole tie-mask plane of
every pair) and ``ends`` (end cells of pair 0 for ``traceback_from``, or None).

The shape arithmetic of pw_strip.h is restated here in Python (``strip_count`` .. ``fixup_segments``); the constants it
rests on are read out of the source text by test_strip_cases.py::test_the_constants_are_the_kernels.
"""
import importlib.util
import os
from functools import lru_cache

import numpy as np

from biseqt_amd import synth

_spec = importlib.util.spec_from_file_location('strip_check', os.path.join(os.path.dirname(__file__), 'micro', 'strip_check.py'))
strip_check = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(strip_check)
SCORES = strip_check.SCORES
MAT = ([[2, -1, -2, -1], [-1, 3, -1, -2], [-2, -1, 2, -1], [-1, -2, -1, 1]], -3, -1)      # (matrix, go, ge)
WALK_SCORE = (1, -3, -5, -2)

GLOBAL, LOCAL, START_ANCHORED, END_ANCHORED, OVERLAP, START_ANCHORED_OVERLAP, END_ANCHORED_OVERLAP = range(7)

# ---- the kernel's constants (test_the_constants_are_the_kernels reads them in the source) ------------------------
STRIP_BLOCK = 32          # kStripBlock: steps per block
STRIP_SUB = 16            # PW_STRIP_SUB: granules per hand-over
FAST_Y = 128              # run(): q_end and `whole` need a.Y > 128
WALK_STRIPS = 4           # PW_WALK_STRIPS
WALK_GROUPS = 5           # kWalkGroups: 32-step groups per strip of the walker's window
FIX_OPS = 2048            # pw_batch_traceback: fix_segments = min(256, max(1, longest tx_cap / 2048))
FIX_MAX = 256
WORKERS = 1024            # launch_strip_fills: PWLIB_STRIP_WAVES
MASK_CELLS = 3 * 10 ** 6  # family 3: whole planes are compared up to this many cells

KINDS = ('0,true', '0,false', '1', '2', '3', '3,true', '4')      # block<MODE[, NOIN]> of run()


def strip_count(X):
    return (X + 1 + 63) // 64


def strip_nkq(Y):
    return (Y + 64 + STRIP_BLOCK - 1) // STRIP_BLOCK


def strip_fifo_pitch(Y):
    return (Y + 1 + 32 + 63) // 64 * 64


def q_last_cell(Y):
    return (Y - STRIP_BLOCK) // STRIP_BLOCK + 1 if Y >= STRIP_BLOCK else 0


def q_end(Y):
    return min(q_last_cell(Y), strip_nkq(Y) - 3) if Y > FAST_Y else 0


def whole(X, Y, w):
    return Y > FAST_Y and 64 * w + 63 <= X


def block_kind(X, Y, w, q):
    """The block template run() instantiates for block q of strip w."""
    if 2 <= q < q_end(Y):
        return '0,true' if w == 0 else '0,false'
    k0 = STRIP_BLOCK * q
    wh = whole(X, Y, w)
    if k0 < 64 and wh:
        return '4' if w > 0 else '1'
    if k0 >= 64 and wh:
        return '3' if w > 0 else '3,true'
    return '2'


def block_kinds(X, Y):
    """The set of block kinds a table of this shape runs."""
    return {block_kind(X, Y, w, q) for w in range(strip_count(X)) for q in range(strip_nkq(Y))}


def fixup_segments(pairs, tx_len):
    """(nseg, seglen) of k_trace_fixup for a transcript of tx_len ops in a batch of these pairs (all on the strips)."""
    longest = max(len(o) + len(m) + 1 for o, m in pairs)
    nseg = min(FIX_MAX, max(1, longest // FIX_OPS))
    return nseg, ((tx_len + nseg - 1) // nseg + 63) & ~63


def runs_of(X, run_len, nq=8):
    """Number of runs the strips of a table are dealt in (run_len None: the default, WORKERS / nq)."""
    rl = run_len if run_len else max(1, WORKERS // nq)
    return (strip_count(X) + rl - 1) // rl


def kw_of(c):
    """The case's problem as the keywords of tests/plane_checks.py (okw_of / bkw_of)."""
    kw = dict(mode=0, alntype=c['alntype'])
    if c['score'] is MAT:
        kw.update(subst=MAT[0], go=MAT[1], ge=MAT[2])
    else:
        mt, ms, go, ge = c['score']
        kw.update(match=mt, mismatch=ms, go=go, ge=ge)
    return kw


def case(cid, family, pairs, alntype, score, run_len=None, masks=True, ends=None, **kw):
    out = dict(id=cid, family=family, pairs=[(np.asarray(o, np.uint8), np.asarray(m, np.uint8)) for o, m in pairs], alntype=alntype,
               score=score, run_len=run_len, masks=masks, ends=ends)
    out.update(kw)
    return out


# ---- sequences -------------------------------------------------------------------------------------------------
START_TYPES = (GLOBAL, START_ANCHORED, START_ANCHORED_OVERLAP)
END_TYPES = (END_ANCHORED, END_ANCHORED_OVERLAP)


def _rand(rng, n):
    return synth.rand_seqs(rng, 1, n)[0] if n > 0 else np.zeros(0, np.uint8)


def related_pair(rng, X, Y, alntype, centre=None, rates=(0.1, 0.04, 0.4)):
    """An origin of X letters and a mutant of exactly Y: a mutated copy of a window of the origin -- at its start for the
    start-anchored types (and GLOBAL), at its end for the end-anchored ones, around row `centre` for LOCAL and OVERLAP --
    cut to Y letters, or filled up with random ones on the side away from the anchor."""
    o = _rand(rng, X)
    L = min(X, Y + Y // 8 + 4)
    if alntype in START_TYPES:
        a = 0
    elif alntype in END_TYPES:
        a = X - L
    else:
        c = X // 2 if centre is None else centre
        a = min(max(c - L // 2, 0), X - L)
    mm = synth.mutate(rng, o[a:a + L], *rates) if L > 0 else np.zeros(0, np.uint8)
    pad = _rand(rng, max(0, Y - len(mm)))
    if alntype in END_TYPES:
        m = np.concatenate([pad, mm])
        m = m[len(m) - Y:]
    else:
        m = np.concatenate([mm, pad])[:Y]
    assert len(m) == Y
    return o, m.astype(np.uint8)


def _score(k):
    return MAT if k % 8 == 7 else SCORES[k % 8]


# ---- family 1: the block-kind grid ---------------------------------------------------------------------------
GRID_X = (63, 64, 127, 128, 129, 300, 700)
GRID_Y = (0, 1, 15, 16, 17, 31, 32, 33, 100, 127, 128, 129, 130, 159, 160, 161, 200, 255, 256, 257, 300)


@lru_cache(None)
def family1():
    """Every (X, Y) of the grid with two alignment types each, rotated so that every type meets every block kind; the
    LOCAL / OVERLAP window sits on the middle strip boundary."""
    out = []
    for xi, X in enumerate(GRID_X):
        for yi, Y in enumerate(GRID_Y):
            for r in range(2):
                t = (xi + yi + 3 * r) % 7
                rng = synth.rng_for(510000 + 1000 * xi + 10 * yi + r)
                centre = 64 * ((X // 64 + 1) // 2)
                o, m = related_pair(rng, X, Y, t, centre)
                out.append(case('grid-%dx%d-t%d' % (X, Y, t), 1, [(o, m)], t, _score(2 * (xi * len(GRID_Y) + yi) + r)))
    return out


# ---- family 2: run boundaries on small tables ----------------------------------------------------------------
def _one_run(X, run):
    return strip_count(X) <= run          # (one run: no boundary)


@lru_cache(None)
def family2():
    out = []
    k = 0
    for X in (129, 300, 700):
        for Y in (100, 128, 129, 300):
            for run in (1, 2, 3):
                if _one_run(X, run):
                    continue
                t = k % 7
                rng = synth.rng_for(520000 + k)
                o, m = related_pair(rng, X, Y, t, 64 * ((X // 64 + 1) // 2))
                out.append(case('run%d-%dx%d-t%d' % (run, X, Y, t), 2, [(o, m)], t, _score(k), run_len=run))
                k += 1
    for Y in (100, 300):
        for t in (GLOBAL, LOCAL, OVERLAP, END_ANCHORED_OVERLAP):
            rng = synth.rng_for(520000 + k)
            o, m = related_pair(rng, 2560, Y, t, 64 * 20)          # 41 strips in runs of 5; the window on the edge of run 3 | 4
            out.append(case('run5-2560x%d-t%d' % (Y, t), 2, [(o, m)], t, _score(k), run_len=5))
            k += 1
    return out


# ---- family 3: run boundary and second draw at the default placement -----------------------------------------
TALL = ((8400, 8192), (16600, 16384))       # (X, the row the homology window straddles): run 0 | 1 and run 1 | 2
TALL_Y = (1, 17, 129, 300)
TALL_TYPES = (GLOBAL, LOCAL, OVERLAP, END_ANCHORED_OVERLAP)
DRAW2 = (66000, 200, 65536)                 # 1032 strips: 8 drawn by wavefronts that have finished one


def _tall_pair(rng, X, Y, row):
    """The mutant is a mutated copy of the origin's letters around `row` -- whatever the type: the end cell and the walk of
    LOCAL / OVERLAP sit on the run boundary, GLOBAL walks a column of D's through every strip."""
    o = _rand(rng, X)
    L = Y + Y // 8 + 4
    a = row - L // 2
    mm = synth.mutate(rng, o[a:a + L], 0.06, 0.02, 0.3)
    m = np.concatenate([mm, _rand(rng, max(0, Y - len(mm)))])[:Y]
    return o, m.astype(np.uint8)


@lru_cache(None)
def family3():
    out = []
    k = 0
    for X, row in TALL:
        for yi, Y in enumerate(TALL_Y):
            for r in range(2):
                t = TALL_TYPES[(yi + 2 * r + (X > 10000)) % 4]
                o, m = _tall_pair(synth.rng_for(530000 + k), X, Y, row)
                out.append(case('tall-%dx%d-t%d' % (X, Y, t), 3, [(o, m)], t, WALK_SCORE if k % 2 == 0 else SCORES[4],
                                masks=(X + 1) * (Y + 1) <= MASK_CELLS, forced=X < 16000))
                k += 1
    X, Y, row = DRAW2
    for t in (GLOBAL, LOCAL):
        o, m = _tall_pair(synth.rng_for(530000 + k), X, Y, row)
        out.append(case('draw2-%dx%d-t%d' % (X, Y, t), 3, [(o, m)], t, WALK_SCORE, masks=False, forced=False))
        k += 1
    return out


# ---- family 4: stale granules inside one batch ---------------------------------------------------------------
@lru_cache(None)
def family4():
    out = []
    for k, t in enumerate((LOCAL, GLOBAL, OVERLAP)):
        rng = synth.rng_for(540000 + k)
        wide = related_pair(rng, 300, 300, t, 128)
        narrow = related_pair(rng, 300, 40, t, 128)
        out.append(case('stale-pitch-t%d' % t, 4, [wide, narrow, wide], t, _score(k)))
        same = [related_pair(rng, 200, 170, t, 64) for _ in range(3)]
        out.append(case('stale-letters-t%d' % t, 4, same, t, _score(k + 3)))
        o, m = related_pair(rng, 260, 190, t, 128)
        out.append(case('stale-swapped-t%d' % t, 4, [(o, m), (m, o), (o, m)], t, _score(k + 5)))
    return out


# ---- family 5: walker windows --------------------------------------------------------------------------------
GAP_EDGES = (159, 160, 161, 255, 256, 257)
IDENTICAL = (62, 63, 64, 65, 127, 128, 700)


def gap_pair(seed, flank, gap, deletion):
    """o = A + B, m = A + G + B (an I run of |G| inside one strip when the flanks are short of a strip boundary), or its mirror
    image (a D run down one column, through |G| / 64 strips).  The first and last letters of G differ from B's first and A's
    last, so the gap cannot slide: the oracle's transcript is M|A| I|G| M|B|."""
    rng = synth.rng_for(seed)
    A, G, B = _rand(rng, flank), _rand(rng, gap), _rand(rng, flank)
    G[0] = (B[0] + 1) % 4
    G[-1] = (A[-1] + 1) % 4
    short, long_ = np.concatenate([A, B]), np.concatenate([A, G, B])
    return (long_, short) if deletion else (short, long_)


def edge_ends(X, Y, seed, sample=200):
    """End cells for traceback_from: the four corners, rows 64 k - 1, 64 k, 64 k + 1 at columns 0, 1, Y - 1, Y, and a sample."""
    ends = [(0, 0), (0, Y), (X, 0), (X, Y)]
    for k in range(1, X // 64 + 1):
        for x in (64 * k - 1, 64 * k, 64 * k + 1):
            if x <= X:
                ends += [(x, y) for y in (0, 1, Y - 1, Y)]
    rng = np.random.default_rng(seed)
    ends += [(int(rng.integers(0, X + 1)), int(rng.integers(0, Y + 1))) for _ in range(sample)]
    return ends


@lru_cache(None)
def family5():
    """All GLOBAL / 1, -3, -5, -2.  The end cells for ``traceback_from`` (``edge_ends``) are attached to two tables only, the
    I run of 161 steps and the D run of 257 rows -- each one past the window: the 300-long runs and the identical pairs are
    walked from the corner alone, and no LOCAL table is walked from explicit ends here (tests/test_gpu_whole_plane.py does
    that for the other types on the strips)."""
    out = []
    for d in (False, True):
        o, m = gap_pair(550000 + d, 400, 300, d)
        out.append(case('walk-%s300' % ('D' if d else 'I'), 5, [(o, m)], GLOBAL, WALK_SCORE, gap=300, flank=400, op='D' if d else 'I'))
    for k, g in enumerate(GAP_EDGES):
        for d in (False, True):
            o, m = gap_pair(550010 + 2 * k + d, 100, g, d)
            # (the ends: on the two tables whose run is one past the window, 161 steps and 257 rows)
            ends = edge_ends(len(o), len(m), 5500 + g) if (g, d) in ((161, False), (257, True)) else None
            out.append(case('walk-%s%d' % ('D' if d else 'I', g), 5, [(o, m)], GLOBAL, WALK_SCORE, ends=ends, gap=g, flank=100,
                            op='D' if d else 'I'))
    for n in IDENTICAL:
        o = _rand(synth.rng_for(550100 + n), n)
        out.append(case('walk-identical-%d' % n, 5, [(o, o.copy())], GLOBAL, WALK_SCORE))
    return out


# ---- family 6: fix-up segments -------------------------------------------------------------------------------
FIX_SIZES = (2047, 2048, 2049, 3071, 3072, 3073)


def _light(rng, o):
    """A lightly mutated copy of the same length."""
    mm = synth.mutate(rng, o, 0.03, 0.003, 0.3)
    return np.concatenate([mm, _rand(rng, max(0, len(o) - len(mm)))])[:len(o)].astype(np.uint8)


@lru_cache(None)
def family6():
    """Identical and lightly mutated pairs at every size, GLOBAL and LOCAL (24 pairs), the pair beside a short one and the
    pair with indels in front of a cut."""
    out = []
    for k, n in enumerate(FIX_SIZES):
        rng = synth.rng_for(560000 + n)
        o = _rand(rng, n)
        out.append(case('fix-identical-%d-global' % n, 6, [(o, o.copy())], GLOBAL, WALK_SCORE, masks=False))
        out.append(case('fix-mutated-%d-local' % n, 6, [(o, _light(rng, o))], LOCAL, WALK_SCORE, masks=False))
        out.append(case('fix-identical-%d-local' % n, 6, [(o, o.copy())], LOCAL, WALK_SCORE, masks=False))
        out.append(case('fix-mutated-%d-global' % n, 6, [(o, _light(rng, o))], GLOBAL, WALK_SCORE, masks=False))
    rng = synth.rng_for(560100)
    o = _rand(rng, 2048)
    m = _light(rng, o)
    # the short pair's transcript is cut into the long one's segments: all but its first are empty
    out.append(case('fix-beside-a-short-pair', 6, [(o, m), (m[:50], o[:60])], LOCAL, WALK_SCORE, masks=False))
    # LOCAL, starting away from (0, 0); indels in the 128 ops in front of the second segment (tx_len ~ 2100, seglen 1088)
    core = _rand(rng, 2100)
    mc = np.concatenate([core[:980], core[983:1010], _rand(rng, 2), core[1010:1050], core[1052:1070], _rand(rng, 1), core[1070:]])
    out.append(case('fix-indels-before-a-cut', 6, [(np.concatenate([_rand(rng, 150), core]), np.concatenate([_rand(rng, 100), mc]))],
                    LOCAL, WALK_SCORE, masks=False))
    return out


FAMILIES = {1: family1, 2: family2, 3: family3, 4: family4, 5: family5, 6: family6}


def cases(family=None):
    if family is not None:
        return list(FAMILIES[family]())
    return [c for f in sorted(FAMILIES) for c in FAMILIES[f]()]
