"""Generates tests/golden/blot_multi_wide.json.gz: the multiple-sequence Word-Blot of the REFERENCE at the sequence
counts that blot_multi.json.gz stops short of, N = 7 and 9 .. 16.  The reference is loaded, run and recorded exactly as
make_blot_multi_golden.py does (whose helpers are imported; blot_multi.json.gz is not touched), and the record layout
is the same, so tests/test_blot_multi_gpu.py holds both files to the same assertions.

    python tests/golden/make_blot_multi_wide_golden.py

What differs is the inputs.  A k-mer must survive in all N sequences to give a seed, so the mutation rate falls as N
grows (0.1 / N, split evenly between substitutions and indels), and a repeated k-mer multiplies through every sequence:
the reference's in-memory class enumerates `itertools.product` in Python and answers `find_all_neighbors` from a
cKDTree, which takes minutes or exhausts memory once a case has tens of thousands of rows.  Every case is therefore
redrawn from the same generator until it has between 50 and 3000 rows; the count is asserted.  The file is written with a
zero gzip timestamp: a second run reproduces it byte for byte.
"""
import gzip
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_blot_golden import hx, load_reference, mutate                         # noqa: E402
from make_blot_multi_golden import boxes, rand, ref_count, segments             # noqa: E402

MIN_ROWS, MAX_ROWS = 50, 3000


def make_case(rng, N, n, hom, kind):
    if kind == 'identical':
        s = rand(rng, n)
        return [list(s) for _ in range(N)]
    if kind == 'unrelated':
        return [rand(rng, n + int(rng.integers(0, 3))) for _ in range(N)]
    core = rand(rng, hom)
    seqs = []
    for _ in range(N):
        pre = int(rng.integers(0, max(1, n - hom)))
        seqs.append(rand(rng, pre) + mutate(rng, core, .05 / N, .05 / N) + rand(rng, max(0, n - hom - pre)))
    return seqs


def count_rows(seqs, w):
    """Rows the case will have (product of the hit counts per shared k-mer), without enumerating them."""
    hits = []
    for s in seqs:
        h = {}
        for i in range(len(s) - w + 1):
            h[tuple(s[i:i + w])] = h.get(tuple(s[i:i + w]), 0) + 1
        hits.append(h)
    total = 0
    for k in hits[0]:
        p = 1
        for h in hits:
            p *= h.get(k, 0)
        total += p
    return total


def cases(RS, RB):
    rng = np.random.default_rng(20261018)
    A = RS.Alphabet('ACGT')
    specs = [  # (N, length, homologous length, wordlen, kind, K, K_min, p_min)
        (7, 400, 200, 8, 'homologous', 80, 80, .6), (9, 400, 200, 8, 'homologous', 80, 80, .6),
        (10, 300, 150, 7, 'homologous', 60, 60, .6), (11, 400, 200, 8, 'homologous', 80, 80, .6),
        (12, 300, 150, 8, 'homologous', 60, 60, .6), (13, 400, 200, 9, 'homologous', 80, 80, .6),
        (14, 300, 160, 8, 'homologous', 60, 60, .6), (15, 400, 200, 8, 'homologous', 80, 80, .6),
        (16, 400, 200, 8, 'homologous', 80, 80, .6), (9, 6, 0, 1, 'unrelated', 3, 3, .3),
        (10, 150, 0, 6, 'identical', 40, 40, .6), (16, 250, 120, 10, 'homologous', 50, 50.5, .65),
    ]
    out = []
    for ci, (N, n, hom, w, kind, K, K_min, p_min) in enumerate(specs):
        t0 = time.time()
        draws = 0
        while True:
            draws += 1
            seqs = make_case(rng, N, n, hom, kind)
            if MIN_ROWS <= count_rows(seqs, w) <= MAX_ROWS:
                break
            assert draws < 200, 'case %d never lands between %d and %d rows' % (ci, MIN_ROWS, MAX_ROWS)
        g_max, sens = .2, .95 if ci % 2 else .9
        WB = RB.WordBlotMultipleFast(*[RS.Sequence(A, s) for s in seqs], wordlen=w, alphabet=A, g_max=g_max,
                                     sensitivity=sens)
        rows = [list(ds) + [a] for ds, a in WB.seeds()]
        assert MIN_ROWS <= len(rows) <= MAX_ROWS
        rec = {'seqs': [''.join('ACGT'[c] for c in s) for s in seqs], 'wordlen': w, 'g_max': hx(g_max),
               'sensitivity': hx(sens), 'kind': kind, 'rows': rows}
        rec['counts'] = [{'ds_band': ds, 'a_band': a, 'count': ref_count(WB, ds, a)} for ds, a in boxes(rng, rows, N)]
        rec['score_seeds'] = {'K': K, 'records': [{'seed': list(r['seed'][0]) + [r['seed'][1]], 'neighs': sorted(r['neighs']),
                                                   'p': hx(r['p'])} for r in WB.score_seeds(K)]}
        rec['similar_segments'] = {'K_min': K_min, 'p_min': hx(p_min),
                                   'plain': segments(WB, K_min, p_min, False, N),
                                   'at_least_one': segments(WB, K_min, .999999, True, N)}
        out.append(rec)
        print('case %d: N=%d w=%d kind=%s rows=%d segments=%d draws=%d (%.1f s)'
              % (ci, N, w, kind, len(rows), len(rec['similar_segments']['plain']), draws, time.time() - t0))
    return out


def main():
    t0 = time.time()
    RS, RB = load_reference()
    src = 'generated by tests/golden/make_blot_multi_wide_golden.py from the reference\'s biseqt/blot.py and seeds.py run ' \
          'under python %d.%d (stub apsw, sha1 wrapper: see make_blot_golden.py)' % sys.version_info[:2]
    data = {'source': src, 'cases': cases(RS, RB)}
    with open(os.path.join(HERE, 'blot_multi_wide.json.gz'), 'wb') as raw:
        with gzip.GzipFile(filename='', mode='wb', fileobj=raw, mtime=0) as f:
            f.write(json.dumps(data).encode('ascii'))
    print('wrote blot_multi_wide.json.gz in %.1f s' % (time.time() - t0))


if __name__ == '__main__':
    main()
