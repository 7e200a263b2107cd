"""Generates tests/golden/planner_decisions.json.gz: what the host planner (`pw_plan_only`, through
`biseqt_amd.batch.plan_only`) decides for a fixed grid of batches, so that a change of the planner's code that is meant to
change no decision can be checked against every one of them (tests/test_planner_golden.py replays the records).

    python tests/golden/make_planner_golden.py

The grid straddles every threshold the planner tests -- a case just inside and one just outside -- over both modes, every
alignment type, alphabet sizes, the sign lattice of match / mismatch / go / ge, small and large substitution matrices, dyadic
and non-dyadic fractions, the 16-bit admission bounds of the packed kernels, band widths, batch sizes, every flag the planner
reads and every planner knob (PWLIB_*) at a non-default value.  A record holds its inputs and the whole returned dict (or the
error message); knobs are set for one record and restored after it.  The file is written deterministically (sorted keys, gzip
without a timestamp): a rerun on the same planner reproduces it byte for byte.
"""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, 'planner_decisions.json.gz')

STD, BANDED = 0, 1
STD_TYPES = range(7)          # GLOBAL, LOCAL, START_ANCHORED, END_ANCHORED, OVERLAP, START_ANCHORED_OVERLAP, END_ANCHORED_OVERLAP
BANDED_TYPES = range(3)       # B_GLOBAL, B_LOCAL, B_OVERLAP
ALL_TYPES = [(STD, t) for t in STD_TYPES] + [(BANDED, t) for t in BANDED_TYPES]
FLAGS = (1, 2, 4, 8, 16, 32, 64, 128, 256)      # every PW_FLAG_* (include/pw_batch.h)
KNOBS = [('PWLIB_NO_DYADIC', '1'), ('PWLIB_LATENCY_MODE', '0'), ('PWLIB_LATENCY_MODE', '1'), ('PWLIB_NO_PACKED_MAT', '1'),
         ('PWLIB_NO_PACKED_ANCHORED', '1'), ('PWLIB_NO_PACKED_OVERLAP', '1'), ('PWLIB_NO_PACKED_MW', '1'),
         ('PWLIB_NO_STRIP', '1'), ('PWLIB_NO_SMALL_STRIP', '1'), ('PWLIB_STRIP_NO_BYTE_ROWS', '1'),
         ('PWLIB_NO_SMALL_TILED', '1'), ('PWLIB_MW_WIDE_LANES', '1'), ('PWLIB_SIMPLE_AS_MATRIX', '0'),
         ('PWLIB_SIMPLE_AS_MATRIX', '1'), ('PWLIB_NO_SCALED16', '1'), ('PWLIB_PACKED_BK', '4'), ('PWLIB_PACKED_BK', '8'),
         ('PWLIB_PACKED_BK', '16'), ('PWLIB_PACKED_BK', '32'), ('PWLIB_PACKED_BK', '4s'), ('PWLIB_PACKED_BK', '8s'),
         ('PWLIB_PACKED_BK', '12s')]
KNOB_NAMES = sorted({k for k, _ in KNOBS})

CFG = (1, -3, -5, -2)                                               # match, mismatch, go, ge
BLASTISH = [[1, -3, -2, -3], [-3, 1, -3, -2], [-2, -3, 1, -3], [-3, -2, -3, 1]]


def simple(match, mismatch, go, ge):
    return dict(match=match, mismatch=mismatch, go=go, ge=ge)


def matrix(S, go=-5, ge=-2):
    return dict(subst=[list(r) for r in S], go=go, ge=ge)


def span_matrix(L, lo, hi):
    """A matrix over L letters whose entries run from lo to hi (diagonal hi, one entry lo, the rest in between): not simple."""
    mid = (lo + hi) // 2 if (lo + hi) // 2 != lo else hi
    return [[hi if i == j else (lo if (i, j) == (0, 1) else mid - (i + j) % 2) for j in range(L)] for i in range(L)]


def banded(n, X, Y, dmin, dmax):
    return [[n, X, Y, dmin, dmax]]


def std(n, X, Y):
    return [[n, X, Y, 0, 0]]


def expand(shapes):
    out = []
    for n, X, Y, dmin, dmax in shapes:
        out += [(X, Y, dmin, dmax)] * n
    return out


def plan(rec):
    """The planner's decision for one record's inputs (its knobs set for the call only) -- or its error message."""
    from biseqt_amd.batch import plan_only
    saved = {k: os.environ.pop(k) for k in KNOB_NAMES if k in os.environ}
    os.environ.update(rec['env'])
    try:
        sc = rec['scores']
        kw = dict(go_score=sc['go'], ge_score=sc['ge'])
        if 'subst' in sc:
            kw.update(subst_scores=sc['subst'], alphabet_len=len(sc['subst']))
        else:
            kw.update(match_score=sc['match'], mismatch_score=sc['mismatch'], alphabet_len=rec['L'])
        return plan_only(expand(rec['shapes']), alnmode=rec['mode'], alntype=rec['type'], flags=rec['flags'], **kw)
    except RuntimeError as e:
        return dict(error=str(e))
    finally:
        for k in rec['env']:
            os.environ.pop(k, None)
        os.environ.update(saved)


def grid():
    recs = []

    def add(mode, typ, scores, shapes, L=4, flags=0, env=None):
        if 'subst' in scores:
            L = len(scores['subst'])
        recs.append(dict(mode=mode, type=typ, L=L, scores=scores, shapes=shapes, flags=flags, env=dict(env or {})))

    def all_types(scores, std_shapes, banded_shapes, **kw):
        for mode, t in ALL_TYPES:
            for sh in (std_shapes if mode == STD else banded_shapes):
                add(mode, t, scores, sh, **kw)

    # ---- the sign lattice: match, mismatch, go, ge each negative, 0 and positive (match == mismatch, mismatch > match,
    #      mismatch > 0 among them), every type, narrow and wide bands, few and many pairs
    lat_std = [std(40, 300, 310), std(2, 3000, 3000), std(600, 1000, 1000)]
    lat_banded = [banded(40, 500, 510, -50, 50), banded(300, 2000, 2000, -1500, 1500), banded(3000, 400, 410, -20, 20)]
    for m in (-1, 0, 2):
        for mm in (-3, 0, 1):
            for go in (-5, 0, 2):
                for ge in (-2, 0, 1):
                    all_types(simple(m, mm, go, ge), lat_std, lat_banded)

    # ---- alphabet sizes (L = 1: only the match score occurs; 4: the packed matrix limit; 32: the LDS table; 33: beyond)
    for L in (1, 2, 4, 5, 20, 32, 33):
        sets = [simple(*CFG), simple(2, 1, -5, -2), simple(3, -1, 0, -1)]
        if L >= 2:
            sets += [matrix(span_matrix(L, -3, 2)), matrix(span_matrix(L, -60, 60), go=-2, ge=-1)]
        for sc in sets:
            all_types(sc, [std(40, 300, 310), std(1, 3000, 3000)], [banded(2000, 1000, 1010, -100, 100), banded(5, 3000, 3000, -1500, 1500)],
                      L=L)

    # ---- matrices: minimum 0 / 1, range 127 / 128 (the byte rows), range 31 / 32 (the scores-times-4 form: 4 range <= 127)
    for L in (2, 3, 4):
        for lo, hi in ((0, 5), (1, 5), (-63, 64), (-64, 64), (-27, 4), (-28, 4), (-31, 0), (-32, 0), (-126, 1), (-127, 1)):
            all_types(matrix(span_matrix(L, lo, hi), go=-3, ge=-1),
                      [std(1500, 400, 400), std(2, 3000, 3000)],
                      [banded(2000, 500, 505, -60, 60), banded(30, 500, 505, -60, 60), banded(100, 3000, 3000, -1500, 1500),
                       banded(3000, 2000, 2010, -400, 400)])
    all_types(matrix(BLASTISH), [std(5000, 1000, 1000)], [banded(3000, 2000, 2010, -400, 400), banded(10000, 2000, 2010, -200, 200)])

    # ---- dyadic and non-dyadic fractions; |score| around the dyadic cap of 1e6; shifts 10 / 11
    for sc in (simple(0.25, -1, 0, -1), simple(3 / 7, -1, 0, -1), simple(1 / .7 - 1, -1, 0, -1), simple(1, -3, -0.5, -0.125),
               simple(0.25, -999999.75, 0, -1), simple(0.25, -1000000.25, 0, -1), simple(2 ** -10, -1, 0, -1),
               simple(2 ** -11, -1, 0, -1), matrix([[0.5, -1.25], [-1, 0.75]]), matrix([[0.3, -1], [-1, 0.3]])):
        all_types(sc, [std(1, 8000, 8000), std(300, 500, 500)], [banded(50, 12000, 12100, -300, 300), banded(3000, 1000, 1000, -20, 20)])

    # ---- the 16-bit admission bounds
    local = [(BANDED, 1), (STD, 1)]
    for n in (300, 3000):
        # maxmin * max(smax, 0) = 2047 / 2048 (rule 3) and 8000 / 8001 (rules 0, 4), with matrices as well
        for X in (2047, 2048, 8000, 8001):
            for sc in (simple(*CFG), matrix(span_matrix(4, -20, 1))):
                add(BANDED, 1, sc, banded(n, X, X + 10, -100, 100))
                add(BANDED, 1, sc, banded(n, X, X + 10, -1200, 1200))
                add(STD, 3, sc, std(n, X, min(X + 10, 8100)))
        for X, m in ((1000, 8), (1001, 8), (1023, 2), (1024, 2)):
            for mode, t in local:
                add(mode, t, simple(m, -3, -5, -2), banded(n, X, X + 10, -100, 100) if mode else std(n, X, X + 10))
        # rule 5: highest <= 8000
        for X, m in ((8000, 1), (8001, 1), (2000, 4), (2001, 4)):
            add(STD, 2, simple(m, -3, -5, -2), std(n, X, min(X + 10, 8100)))
            add(STD, 2, simple(m, -3, -5, -2), std(n // 100, X, min(X + 10, 8100)))
        # ... where it is the only bound that decides: 7998 / 8001 (lowest about 18 700)
        for X in (2666, 2667):
            add(STD, 2, simple(3, -3, -5, -2), std(n, X, X + 10))
        # maxspan = X + Y + 2 = 31999 / 32000 (steps as signed 16 bits) where it is the only bound that decides: rule 0 with
        # the best score at 8000, rules 1 / 2 with every score within [-16 300, 16 000]
        for Y in (23997, 23998):
            add(BANDED, 1, simple(*CFG), banded(n, 8000, Y, -100, 100))
        for X in (15998, 15999):
            for t in (0, 2):
                add(BANDED, t, simple(1, -1, -2, -1), banded(n, X, 15999, -100, 100))
        # rules 1 / 2: lowest = maxmin * max(-smin, 0) + |go| + |ge| (maxnd + 2) = 23000 / 23001 ...
        for t in (0, 2):
            for half in (494, 495):      # 988 / 990 diagonals
                add(BANDED, t, simple(1, -10, -10, -1), banded(n, 2200, 2200, -half, 493 if t == 2 else half))
                add(BANDED, t, simple(1, -10, -10, -1), banded(n, 2200, 2200, -half, 494))
            for X in (2299, 2300, 2301):
                add(BANDED, t, simple(1, -10, -10, -1), banded(n, X, X, -343, 343))
            # ... highest = maxmin * max(smax, 0) = 30000 / 30001 (and 29982 / 30030)
            for X, m in ((1000, 30), (1001, 30), (1578, 19), (1579, 19)):
                add(BANDED, t, simple(m, -1, -2, -1), banded(n, X, X, -100, 100))
                add(BANDED, t, matrix(span_matrix(4, -1, m), go=-2, ge=-1), banded(n, X, X, -100, 100))
        for X, m in ((1000, 30), (1579, 19), (2299, 1), (2301, 1)):
            for t in (0, 4, 5, 6):
                add(STD, t, simple(m, -10, -10, -1), std(n, X, X))
        # maxabs 100 / 101 (|go + ge|, a substitution score)
        for sc in (simple(1, -3, -98, -2), simple(1, -3, -99, -2), simple(100, -3, -5, -2), simple(101, -3, -5, -2),
                   simple(1, -100, -5, -2), simple(1, -101, -5, -2)):
            for mode, t in ALL_TYPES:
                add(mode, t, sc, banded(n, 40, 41, -20, 20) if mode else std(n, 40, 41))
        # maxspan = X + Y + 2: 31999 / 32000 on every type; maxspan * maxabs: 2^25 (strips), 2^27 (i32 / f64)
        for XY in (31997, 31998):
            for mode, t in ALL_TYPES:
                add(mode, t, simple(*CFG), banded(n // 100, XY // 2, XY - XY // 2, -200, 200) if mode else std(1, XY // 2, XY - XY // 2))
        for XY, sc in ((32765, simple(1, -1, -1023, -1)), (32766, simple(1, -1, -1023, -1)),
                       (32765, simple(1, -1, -4095, -1)), (32766, simple(1, -1, -4095, -1))):
            for mode, t in ALL_TYPES:
                add(mode, t, sc, banded(n // 100, XY // 2, XY - XY // 2, -200, 200) if mode else std(1, XY // 2, XY - XY // 2))

    # ---- band widths: maxnd 1024 / 1025 (tiles), 2048 / 2049 (one wavefront), 16384 / 16385 (a workgroup)
    for nd in (1024, 1025, 2048, 2049, 16384, 16385):
        lo = -(nd // 2)
        for n in (1, 10, 300):
            for sc in (simple(*CFG), simple(0.3, -1.1, -2, -0.7), matrix(BLASTISH), matrix(span_matrix(5, -3, 2))):
                for t in BANDED_TYPES:
                    add(BANDED, t, sc, banded(n, 20000, 20000, lo, lo + nd - 1))
    # ---- batch sizes: 256 / 257 solvable pairs (latency mode), 1024 / 1025, and the side-by-side window above them
    for n in (256, 257, 1024, 1025, 2000, 4096, 8192, 20000):
        for sh in (banded(n, 1000, 1000, -10, 10), banded(n, 2000, 2010, -200, 200), banded(n, 1000, 1000, -300, 300),
                   banded(n, 2000, 2000, -700, 700)):
            for t in BANDED_TYPES:
                add(BANDED, t, simple(*CFG), sh)
        if n <= 2000:
            for t in STD_TYPES:
                add(STD, t, simple(*CFG), std(n, 400, 410))
    # ---- strips: the shortest origin of a few standard-mode pairs, 126 / 127
    for X in (126, 127):
        for n in (1, 4, 16):
            for sc in (simple(*CFG), matrix(BLASTISH), matrix(span_matrix(4, -128, 127)), matrix(span_matrix(4, -129, 127))):
                for t in STD_TYPES:
                    add(STD, t, sc, std(n - 1, 3000, 3000) + std(1, X, 3000) if n > 1 else std(1, X, 3000))
    # ---- mixed batches: band widths, shapes, unsolvable pairs (B_GLOBAL off the end diagonal, an empty band)
    mixed = [banded(100, 500, 500, -10, 10) + banded(100, 2000, 2000, -600, 600),
             banded(3000, 300, 300, -10, 10) + banded(5, 20000, 20000, -3000, 3000),
             banded(500, 1000, 1000, -10, 10) + banded(200, 1000, 1100, 200, 300) + banded(10, 50, 50, 10, -10),
             banded(2, 100, 100, 5, 10) + banded(2, 100, 200, -3, 3),
             banded(300, 100, 200, 5, 10),
             banded(0, 0, 0, 0, 0),
             banded(10, 0, 0, 0, 0) + banded(10, 0, 50, -60, 60)]
    for sh in mixed:
        for sc in (simple(*CFG), simple(0.3, -1.1, -2, -0.7), matrix(BLASTISH)):
            for t in BANDED_TYPES:
                add(BANDED, t, sc, sh)
    for sh in (std(10, 0, 0) + std(10, 5, 0), std(3, 0, 3000) + std(1, 3000, 3000), std(50, 10, 10) + std(2, 8000, 8000),
               std(1000, 300, 300) + std(1, 20000, 20000)):
        for sc in (simple(*CFG), simple(0.3, -1.1, -2, -0.7), matrix(BLASTISH)):
            for t in STD_TYPES:
                add(STD, t, sc, sh)

    # ---- flags and knobs on representative batches
    reps = [(STD, 0, simple(*CFG), std(1, 1000, 1000)),
            (BANDED, 1, simple(*CFG), banded(10000, 2000, 2010, -200, 200)),
            (BANDED, 1, simple(*CFG), banded(20000, 300, 300, -10, 10)),
            (BANDED, 2, simple(*CFG), banded(2000, 5000, 5000, 2700, 3300)),
            (BANDED, 2, simple(*CFG), banded(2000, 1000, 1000, -10, 10)),
            (STD, 1, simple(*CFG), std(4, 2000, 2000)),
            (STD, 1, simple(*CFG), std(1, 100000, 100218)),
            (STD, 2, simple(*CFG), std(1000, 500, 510)),
            (STD, 3, simple(*CFG), std(1000, 500, 510)),
            (STD, 4, simple(*CFG), std(600, 1000, 1000)),
            (BANDED, 1, matrix(BLASTISH), banded(3000, 2000, 2010, -400, 400)),
            (BANDED, 0, simple(0.3, -1.1, -2, -0.7), banded(3000, 3000, 3000, -600, 600)),
            (BANDED, 0, simple(0.25, -1, 0, -1), banded(50, 12000, 12100, -300, 300)),
            (BANDED, 1, simple(*CFG), banded(300, 10000, 10000, -1500, 1500)),
            (STD, 0, simple(0.3, -1.1, -2, -0.7), std(1, 8000, 8000)),
            (BANDED, 1, simple(*CFG), banded(2000, 1000, 1000, -10, 10)),
            (BANDED, 1, matrix(BLASTISH), banded(10, 1000, 1000, -1100, 1100)),
            (STD, 0, matrix(BLASTISH), std(2, 3000, 3000)),
            (STD, 1, simple(2, 1, -5, -2), std(4, 2000, 2000)),
            (BANDED, 1, simple(2, 1, -5, -2), banded(20, 4000, 4000, -1800, 1800)),
            (BANDED, 1, simple(2, -1, -3, -1), banded(300, 700, 700, -40, 40)),
            (BANDED, 2, matrix(span_matrix(4, -20, 3)), banded(3000, 600, 600, -30, 30)),
            (STD, 6, simple(*CFG), std(600, 1000, 1000)),
            (STD, 5, simple(*CFG), std(3, 3000, 3000)),
            (BANDED, 1, simple(*CFG), banded(50000, 300, 300, -20, 20)),
            (BANDED, 1, simple(*CFG), banded(3000, 2000, 2010, -400, 400))]
    for mode, t, sc, sh in reps:
        for f in FLAGS + (16 | 64, 1 | 32, 2 | 16):
            add(mode, t, sc, sh, flags=f)
        for k, v in KNOBS:
            add(mode, t, sc, sh, env={k: v})
        add(mode, t, sc, sh, env={'PWLIB_LATENCY_MODE': '1', 'PWLIB_NO_SMALL_STRIP': '1', 'PWLIB_NO_PACKED_MW': '1'})
        add(mode, t, sc, sh, env={'PWLIB_PACKED_BK': '8s', 'PWLIB_LATENCY_MODE': '1'})
    return recs


def main():
    recs = grid()
    for r in recs:
        r['out'] = plan(r)
    data = json.dumps(recs, sort_keys=True, separators=(',', ':')).encode()
    with open(OUT, 'wb') as f, gzip.GzipFile(filename='', mode='wb', fileobj=f, mtime=0) as g:
        g.write(data)
    kinds = {}
    for r in recs:
        k = r['out'].get('kernel', 'error').split('<')[0]
        kinds[k] = kinds.get(k, 0) + 1
    print('%d records -> %s; %s' % (len(recs), OUT, sorted(kinds.items())))


if __name__ == '__main__':
    main()
