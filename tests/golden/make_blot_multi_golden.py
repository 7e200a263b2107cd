"""Generates tests/golden/blot_multi.json.gz from the REFERENCE's own multiple-sequence Word-Blot
(`/root/reference/biseqt/blot.py:1040-1083`, `WordBlotMultipleFast`, and the classmethods of `seeds.py:SeedIndexMultiple`),
imported in the build container only, the way make_blot_golden.py does (`load_reference`: stub apsw, sha1 wrapper).

    python tests/golden/make_blot_multi_golden.py

Inputs are built with numpy (letters as integers, the same mutation model as make_blot_golden.py) and handed to the
reference as its own Sequence objects; the reference's `stochastics.py` is never imported.  Per case the fixture holds
the full `seeds()` list, `seed_count` on random hyper-boxes (a None sub-bound is handed to the reference, whose in-memory
`seed_count` cannot take one, as a bound wider than every seed), `score_seeds` (seed, sorted neighbours, `p` as hex) and
`similar_segments` with and without `at_least_one`.  Besides: `to_ij_coordinates_seg` on random segments and the
MemoryError boundary of the constructor.

Python-2-only semantics (the reference is python 2; this runs it under python 3):
  * `to_ij_coordinates` divides `a + sum(d)` by N with `/` (seeds.py:287): python 2 floors.  A record whose corners do
    not all divide evenly carries `"py2_safe": false`; its python-2 value is the floor of every coordinate recorded here.
  * `K_hat = ceil((a_max - a_min) / N)` in `similar_segments` (blot.py:1016) is, under python 2, `(a_max - a_min) // N`.
    Segments whose width is not a multiple of N carry `"scores_py2_safe": false`; their `scores` are not compared.
"""
import gzip
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_blot_golden import hx, load_reference, mutate   # noqa: E402

BIG = 10 ** 9      # a bound no seed reaches: the reference's stand-in for an unbounded coordinate


def rand(rng, n):
    return [int(v) for v in rng.integers(0, 4, n)]


def make_case(rng, N, n, hom, w, kind):
    """N sequences of about n letters: `hom` letters of a shared segment at random offsets (homologous), none
    (unrelated), or N copies of one sequence (identical); 'short' makes the last sequence shorter than the word."""
    if kind == 'identical':
        s = rand(rng, n)
        return [list(s) for _ in range(N)]
    if kind == 'unrelated':
        return [rand(rng, n + int(rng.integers(0, 40))) for _ in range(N)]
    core = rand(rng, hom)
    seqs = []
    for _ in range(N):
        pre = int(rng.integers(0, max(1, n - hom)))
        seqs.append(rand(rng, pre) + mutate(rng, core, .03, .03) + rand(rng, max(0, n - hom - pre)))
    if kind == 'short':
        seqs[-1] = rand(rng, w - 1)
    return seqs


def boxes(rng, rows, N):
    out = []
    for _ in range(12):
        if len(rows) and rng.random() < 0.7:
            c = rows[int(rng.integers(0, len(rows)))]
        else:
            c = [int(v) for v in rng.integers(-500, 500, N - 1)] + [int(rng.integers(0, 3000))]
        ds = []
        for k in range(N - 1):
            if rng.random() < 0.25:
                ds.append(None)
            else:
                r = int(rng.integers(0, 60))
                ds.append([c[k] - r, c[k] + int(rng.integers(0, 60))])
        a = None if rng.random() < 0.2 else [c[-1] - int(rng.integers(0, 400)), c[-1] + int(rng.integers(0, 400))]
        if rng.random() < 0.1:
            ds = None
        out.append((ds, a))
    return out


def ref_count(WB, ds, a):
    ds_ref = None if ds is None else [tuple(b) if b is not None else (-BIG, BIG) for b in ds]
    return WB.seed_count(ds_band=ds_ref, a_band=tuple(a) if a is not None else None)


def segments(WB, K_min, p_min, at_least_one, N):
    out = []
    for s in WB.similar_segments(K_min, p_min, at_least_one=at_least_one):
        ds, a = s['segment']
        out.append({'segment': [[list(d) for d in ds], list(a)], 'p': hx(s['p']),
                    'scores': [hx(s['scores'][0]), hx(s['scores'][1])],
                    'scores_py2_safe': (a[1] - a[0]) % N == 0})
    return out


def cases(RS, RB):
    rng = np.random.default_rng(20261015)
    A = RS.Alphabet('ACGT')
    specs = [  # (N, length, homologous length, wordlen, kind, K, K_min, p_min)
        (2, 400, 200, 5, 'homologous', 100, 100, .5), (2, 300, 0, 4, 'unrelated', 60, 60, .4),
        (3, 300, 150, 5, 'homologous', 80, 80, .5), (3, 200, 0, 3, 'unrelated', 40, 40, .5),
        (3, 120, 0, 4, 'identical', 40, 40, .6), (3, 600, 300, 6, 'homologous', 150, 150, .6),
        (4, 500, 250, 6, 'homologous', 100, 100, .6), (4, 150, 0, 3, 'unrelated', 30, 30, .5),
        (4, 3000, 1200, 8, 'homologous', 600, 600, .7), (5, 800, 400, 7, 'homologous', 200, 200, .6),
        (5, 80, 0, 4, 'identical', 20, 20, .5), (6, 1000, 500, 8, 'homologous', 250, 250, .6),
        (6, 50, 30, 3, 'homologous', 15, 15, .4), (4, 300, 150, 5, 'short', 80, 80, .5),
        (3, 700, 0, 7, 'unrelated', 200, 200, .5), (5, 2000, 1000, 8, 'homologous', 500, 450.5, .65),
    ]
    out = []
    for ci, (N, n, hom, w, kind, K, K_min, p_min) in enumerate(specs):
        seqs = make_case(rng, N, n, hom, w, kind)
        g_max, sens = .2, .95 if ci % 2 else .9
        WB = RB.WordBlotMultipleFast(*[RS.Sequence(A, s) for s in seqs], wordlen=w, alphabet=A, g_max=g_max,
                                     sensitivity=sens)
        rows = [list(ds) + [a] for ds, a in WB.seeds()]
        rec = {'seqs': [''.join('ACGT'[c] for c in s) for s in seqs], 'wordlen': w, 'g_max': hx(g_max),
               'sensitivity': hx(sens), 'kind': kind, 'rows': rows}
        rec['counts'] = [{'ds_band': ds, 'a_band': a, 'count': ref_count(WB, ds, a)} for ds, a in boxes(rng, rows, N)]
        rec['score_seeds'] = {'K': K, 'records': [{'seed': list(r['seed'][0]) + [r['seed'][1]], 'neighs': sorted(r['neighs']),
                                                   'p': hx(r['p'])} for r in WB.score_seeds(K)]}
        rec['similar_segments'] = {'K_min': K_min, 'p_min': hx(p_min),
                                   'plain': segments(WB, K_min, p_min, False, N)}
        if rows:
            rec['similar_segments']['at_least_one'] = segments(WB, K_min, .999999, True, N)
        out.append(rec)
        print('case %d: N=%d w=%d rows=%d segments=%d' % (ci, N, w, len(rows), len(rec['similar_segments']['plain'])))
    return out


def coordinate_maps(RSeeds):
    rng = np.random.default_rng(20261016)
    out = []
    for _ in range(60):
        N = int(rng.integers(2, 7))
        ds = []
        for _k in range(N - 1):
            lo = int(rng.integers(-300, 300))
            ds.append([lo, lo + int(rng.integers(0, 50))])
        a0 = int(rng.integers(0, 4000))
        seg = (ds, [a0, a0 + int(rng.integers(0, 300))])
        res = RSeeds.SeedIndexMultiple.to_ij_coordinates_seg((tuple(tuple(d) for d in ds), tuple(seg[1])))
        safe = all(float(v) == int(v) for rng_ in res for v in rng_)
        out.append({'segment': [ds, seg[1]], 'ij': [[float(v) for v in r] for r in res], 'py2_safe': safe})
    return out


def memory_boundary(RS, RB):
    A = RS.Alphabet('ACGT')
    seqs = [RS.Sequence(A, [0, 1, 2, 3, 0, 1, 2, 3, 0, 1]), RS.Sequence(A, [1, 2, 3, 0, 1, 2, 3, 0, 1, 2])]
    out = []
    for w in (3, 5, 6, 8):
        need = 24. * 4 ** w / 2 ** 30         # python 2's 24-byte int; python 3's is 28: only margins both agree on
        for allowed in (need * .5, need * 1.2, 1):
            try:
                RB.WordBlotMultipleFast(*seqs, wordlen=w, alphabet=A, g_max=.2, sensitivity=.9, allowed_memory=allowed)
                raised = False
            except MemoryError:
                raised = True
            out.append({'wordlen': w, 'allowed_memory': hx(allowed), 'raises': raised})
    return out


def main():
    RS, RB = load_reference()
    import biseqt.seeds as RSeeds
    src = 'generated by tests/golden/make_blot_multi_golden.py from /root/reference/biseqt/blot.py and seeds.py run under ' \
          'python %d.%d (stub apsw, sha1 wrapper: see make_blot_golden.py)' % sys.version_info[:2]
    data = {'source': src, 'cases': cases(RS, RB), 'to_ij_coordinates_seg': coordinate_maps(RSeeds),
            'memory': memory_boundary(RS, RB)}
    with gzip.open(os.path.join(HERE, 'blot_multi.json.gz'), 'wt') as f:
        json.dump(data, f)
    print('wrote blot_multi.json.gz')


if __name__ == '__main__':
    main()
