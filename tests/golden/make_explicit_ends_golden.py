"""Generates tests/golden/explicit_ends.json.gz: ``dptable_traceback(T, end)`` from explicit end cells, recorded from the
REFERENCE library compiled by oracle/Makefile (oracle/_ref/pwlib_ref.so) through oracle/ref_driver.py.

    python tests/golden/make_explicit_ends_golden.py

About 300 problems over the 10 alignment types (7 standard, 3 banded), go < 0, go = 0 and go > 0, sub-frames, bands the
reference clamps and one-diagonal bands, and one float (log-odds) scoring stored as hex; each with 4 - 6 end cells:
(0, 0), cells on the table edges, the first and the last diagonal of the band, a LOCAL cell of score 0 and random
interior cells.  Per end cell the record holds what the reference returns: NULL (``null``) or the transcript, start and
``score`` (hex; ``cells[end].choices[0].score``, pw.c:148).  Cells where the reference cannot be run are recorded as
skipped with the reason, predicted by the oracle (oracle/pw_oracle.c, ``pwo_traceback_from``): ``no_choice`` (the cell
holds no choice: pw.c:123 dereferences NULL) and ``panick`` (pw.c:132-134 exits the process).
"""
import gzip
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import oracle as O          # noqa: E402
from oracle import ref_driver as RD     # noqa: E402

OUT = os.path.join(HERE, 'explicit_ends.json.gz')
_H = float.fromhex
LOGODDS = ([[_H('0x1.6e1f76b4337c7p+0') if i == j else _H('-0x1.b7a5d3c4e7ae1p+0') for i in range(4)] for j in range(4)],
           _H('-0x1.2a0d45b6a4e1cp+1'), _H('-0x1.0a6b4e1e13ec7p-2'))


def enc(seq):
    return ''.join(chr(ord('0') + int(c)) for c in seq)


def problems():
    rng = np.random.default_rng(20261016)
    out = []
    for n in range(300):
        mode = 0 if n % 10 < 7 else 1
        alntype = n % 10 if mode == 0 else n % 10 - 7
        X, Y = int(rng.integers(1, 24)), int(rng.integers(1, 24))
        L = 4
        o = rng.integers(0, L, X + 4)
        m = o[:Y + 4].copy() if Y <= X else np.concatenate([o, rng.integers(0, L, Y - X)])
        m = m[:Y + 4] if len(m) >= Y + 4 else np.concatenate([m, rng.integers(0, L, Y + 4 - len(m))])
        flip = rng.random(len(m)) < 0.25
        m[flip] = rng.integers(0, L, int(flip.sum()))
        kw = dict(mode=mode, alntype=alntype, L=L)
        gsign = n % 3                                   # go < 0, go = 0, go > 0
        kw['match'] = float(rng.choice([1, 2, 3]))
        kw['mismatch'] = float(rng.choice([-1, -2, 0]))
        kw['ge'] = float(rng.choice([-1, -2, -0.5]))
        kw['go'] = [-float(rng.choice([1, 3, 2.5])), 0.0, float(rng.choice([1, 0.5]))][gsign]
        if n % 37 == 5:                                  # one float log-odds scoring (hex in the fixture)
            kw.pop('match'); kw.pop('mismatch')
            kw['subst'], kw['go'], kw['ge'] = LOGODDS
        if n % 4 == 1:                                   # a sub-frame
            kw['origin_range'] = (2, 2 + X)
            kw['mutant_range'] = (1, 1 + Y)
        else:
            o, m = o[:X], m[:Y]
        if mode == 1:
            kind = n % 5
            if kind == 0:
                band = (-Y - 3, X + 5)                   # clamped by the reference
            elif kind == 1:
                d = int(rng.integers(-Y, X + 1))
                band = (d, d)                            # one diagonal
            elif kind == 2:
                band = (min(0, X - Y) - 1, max(0, X - Y) + 1)
            else:
                a, b = sorted(int(v) for v in rng.integers(-Y, X + 1, 2))
                band = (a, b)
            kw['diag_range'] = band
        out.append((o, m, kw))
    return out


def end_cells(res, X, Y, mode, rng):
    """(0, 0), table edges, first and last diagonal, a zero-score cell, random interior cells: 4 - 6 distinct cells."""
    if mode == 0:
        rows = [(i, Y + 1) for i in range(X + 1)]
    else:
        rows = [(i, 1 + min(res['band'][0] + i, 0) + min(X - res['band'][0] - i, Y)) for i in range(res['num_rows'])]
    cells = [(i, j) for i, n in rows for j in range(n)]
    want = [(0, 0), cells[-1], (rows[0][0], rows[0][1] - 1), (rows[-1][0], 0)]
    if mode == 0:
        want += [(X, 0), (0, Y), (X, int(rng.integers(0, Y + 1))), (int(rng.integers(0, X + 1)), Y)]
    H = res.get('H')
    if H is not None:
        zero = [cells[k] for k in range(len(cells)) if H[k] == 0 and cells[k] != (0, 0)]
        if zero:
            want.append(zero[int(rng.integers(0, len(zero)))])
    want += [cells[int(k)] for k in rng.integers(0, len(cells), 3)]
    seen, out = set(), []
    for c in want:
        if c in seen or c[0] >= len(rows) or c[1] >= rows[c[0]][1]:
            continue
        seen.add(c)
        out.append(c)
    return out[:6] if len(out) >= 4 else out


def hx(v):
    return float(v).hex()


def main():
    RD.check_layout()
    lib = RD.load(RD.REF_SO)
    rng = np.random.default_rng(7)
    recs, skipped = [], {'no_choice': 0, 'panick': 0}
    for o, m, kw in problems():
        okw = {k: v for k, v in kw.items() if k not in ('L',)}
        okw['L'] = kw['L']
        full = O.solve(o, m, want_table=True, **okw)
        if full['init_rc'] != 0:
            continue
        X = (kw['origin_range'][1] - kw['origin_range'][0]) if 'origin_range' in kw else len(o)
        Y = (kw['mutant_range'][1] - kw['mutant_range'][0]) if 'mutant_range' in kw else len(m)
        ends = []
        for e in end_cells(full, X, Y, kw['mode'], rng):
            pred = O.traceback_from(o, m, e, **okw)
            if pred['no_choice'] or pred['would_panick']:
                why = 'no_choice' if pred['no_choice'] else 'panick'
                skipped[why] += 1
                ends.append(dict(end=list(e), skipped=why))
                continue
            P = RD.Problem(o, m, mode=kw['mode'], alntype=kw['alntype'], subst=kw.get('subst'), L=kw['L'],
                           match=kw.get('match', 1.), mismatch=kw.get('mismatch', 0.), go=kw['go'], ge=kw['ge'],
                           diag_range=kw.get('diag_range'), origin_range=kw.get('origin_range'),
                           mutant_range=kw.get('mutant_range'))
            r = RD.run(lib, P, end=e)
            if r['opt'] == (-1, -1):
                continue                                 # (the driver traces back only after a found optimum)
            if r['tb_null']:
                ends.append(dict(end=list(e), null=True))
            else:
                ends.append(dict(end=list(e), null=False, transcript=r['transcript'], origin_idx=r['origin_idx'],
                                 mutant_idx=r['mutant_idx'], score=hx(r['tb_score'])))
        if not ends:
            continue
        rk = {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items() if k not in ('subst', 'go', 'ge')}
        rec = dict(origin=enc(o), mutant=enc(m), kw=rk, kw_hex=dict(go=hx(kw['go']), ge=hx(kw['ge']),
                   subst=[[hx(v) for v in row] for row in (kw.get('subst') or
                          [[kw['match'] if i == j else kw['mismatch'] for i in range(kw['L'])] for j in range(kw['L'])])]),
                   ends=ends)
        recs.append(rec)
    doc = dict(generator='tests/golden/make_explicit_ends_golden.py', source='oracle/_ref/pwlib_ref.so via oracle/ref_driver.py',
               skipped=skipped, records=recs)
    raw = json.dumps(doc, sort_keys=True, separators=(',', ':')).encode()
    with open(OUT, 'wb') as f:
        with gzip.GzipFile(fileobj=f, mode='wb', mtime=0, filename='') as g:
            g.write(raw)
    print('%d problems, %d end cells (%s skipped), %d bytes' % (len(recs), sum(len(r['ends']) for r in recs), skipped,
                                                               os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
