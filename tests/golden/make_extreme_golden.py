"""Generate tests/golden/extreme_scores.json from the COMPILED REFERENCE: scores around the reference's -INT_MAX floor.

    python tests/golden/make_extreme_golden.py          (in the build container, where /root/reference exists)

The reference starts every gap candidate's maximum at -INT_MAX (_pw_internals.c:267) and the OVERLAP / B_OVERLAP end-cell
searches too (:320, :381).  These problems put go / ge / mismatch between about +-2e7 and +-3e9, on both sides of
(X + Y + 2) * max|score| = INT_MAX, in every standard and banded alignment type -- among them overlap problems whose every
end cell lies below -INT_MAX, where the reference returns no end cell.  Expected values are outputs of
oracle/_ref/pwlib_ref.so driven by oracle/ref_driver.py (the record format of make_golden.py); the file is data only and a
rerun reproduces it byte for byte."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.make_golden import reference_record   # noqa: E402

INT_MAX = 2147483647


def problems():
    rng = np.random.default_rng(20261015)
    out = []
    origin = rng.integers(0, 4, 50).tolist()
    mutant = origin[:20] + origin[25:]                       # letters 20..24 deleted
    std = [(0, t) for t in range(7)]
    banded = [(1, t) for t in range(3)]
    # the issue's witness and its neighbours: GLOBAL, 1 / -1, go from -2e7 to -3e9
    scores = [(1., -1., -3e9, -1.), (1., -1., -2147483000., -1000.), (1., -1., -2e7, -1.), (1., -1., -22139006., -1.),
              (1., -1., -22139007., -1.), (1., -3e9, -5., -2.), (1., -2.5e7, -5., -2.), (1., -1., -5., -3e9)]
    for k, sc in enumerate(scores):
        for mode, t in (std + banded):
            if (k + t + 3 * mode) % 2:                       # (half of the (scores, type) grid: ~55 problems in all)
                continue
            kw = dict(L=4, mode=mode, alntype=t, match=sc[0], mismatch=sc[1], go=sc[2], ge=sc[3])
            if mode == 1:
                kw['diag_range'] = [-8, 8]
            out.append((origin, mutant, kw))
    # overlap problems whose every end cell lies below -INT_MAX: unrelated letters, a huge mismatch and gap-open score
    # (START_ANCHORED_OVERLAP, B_OVERLAP; a standard OVERLAP begins on the edges, so its bottom-left end cell scores 0);
    # and standard OVERLAP with its best end cell far below zero
    for mode, t, dr in ((0, 5, None), (1, 2, [-3, 3]), (0, 4, None)):
        for mm in (-3e9, -1e9):
            kw = dict(L=4, mode=mode, alntype=t, match=1., mismatch=mm, go=-3e9, ge=-1.)
            if dr:
                kw['diag_range'] = dr
            out.append(([0] * 12, [1] * 12, kw))
    # a go that pushes only the gap candidates under the floor, on both sides of it
    for go in (-2147483600., -2147483700.):
        for mode, t in ((0, 0), (0, 2), (1, 0), (1, 2)):
            kw = dict(L=4, mode=mode, alntype=t, match=2., mismatch=-1., go=go, ge=-30.)
            if mode == 1:
                kw['diag_range'] = [-6, 6]
            out.append((origin[:30], mutant[:28], kw))
    return out


def main():
    recs = [reference_record(o, m, kw) for o, m, kw in problems()]
    with open(os.path.join(HERE, 'extreme_scores.json'), 'w') as f:
        json.dump(dict(source='oracle/_ref/pwlib_ref.so (reference C sources, unmodified) -- scores near -INT_MAX',
                       records=recs), f, indent=0, sort_keys=True)
        f.write('\n')
    print('%d records' % len(recs))


if __name__ == '__main__':
    main()
