"""Shapes shared by the tests of the pair keys (pw_wave.h, WaveFill16, PAIRK; pw_plan.h, pair_keys): the packed kernel of rule 3
in matrix form, 8 diagonals per lane, one pair per wavefront, letters from LDS, takes ONE running-best key for the cells of
iterations k and k + 1 (k even) of a slot -- consecutive cells c, c' of one diagonal -- and the end-cell search finds out which
of the two held the best: c' iff its tie nibble has none of B, D, I and its letters score above 0.

What can go wrong there, and the smallest shape for each:
  * the best in the first and in the second cell of a pair, in the even-step and the odd-step registers, in the low and the
    high half of a register: a single run of matches on diagonals 0, 1, 4, 5 of a band that begins at -8 (slots 0, 1, 4, 5 of
    lane 1), ending at x = 30 and x = 31 -- behind a best in the first cell, c' keeps the diagonal move alone on a MISMATCH;
  * c' with D and I kept: the same run scored 2 / -9 / go 0 / ge -1, where the cell behind the best takes S - 2 from both gaps;
  * the pair at a diagonal's start -- (before the start, edge cell) and (edge cell, best) -- : one matching letter at the
    start of diagonals 0 and 2;
  * the best in a diagonal's last cell, the partner beyond the table: a run that ends at (X, Y), X and Y of both parities;
  * many slots tie on S and the resolved rank decides: A...A against A...A;
  * no match at all (S = 0: no stamp, nothing to resolve);
  * the key's top: best score 2047;
  * the last group holds 0 .. 3 blocks (mod 4) and the best rises in it: a run that ends in the pair's last cell;
  * a pair shorter than a block;
  * config 2's table shape, 400 x 390, at band radius 20 and 200;
  * a 4 x 4 matrix with positive entries off its diagonal.
"""
import numpy as np

from tests import ramp_free_cases as RC
from tests import stamp_group_cases as SC

CFG2 = (1., -3., -5., -2.)                 # (match, mismatch, go, ge)
GAPS = (2., -9., 0., -1.)


def cfg2_matrix():
    return RC.matrix(CFG2[0], CFG2[1])


def gaps_matrix():
    return RC.matrix(GAPS[0], GAPS[1])


def mixed_matrix():
    """Match 5, mismatch -4, and three positive entries off the diagonal; no entry 0, range 9 (36 times 4)."""
    S = [[-4.0] * 4 for _ in range(4)]
    for i in range(4):
        S[i][i] = 5.0
    S[0][1] = S[1][0] = 2.0
    S[2][3] = 1.0
    return S


def s0_of(shape):
    """Step 0's anti-diagonal x + y (WaveFill16::run)."""
    _, o, m, band = shape
    dmin, dmax = max(band[0], -len(m)), min(band[1], len(o))
    amin = dmin if dmin > 0 else (-dmax if dmax < 0 else 0)
    return amin - (amin - dmin) % 2


def iteration_of(shape, x, y):
    """The iteration on which a slot holds cell (x, y): even -- the first cell of a key's pair, odd -- the second."""
    return (x + y - s0_of(shape)) >> 1


def slot_of(shape, d):
    _, o, m, band = shape
    return (d - max(band[0], -len(m))) % 8


def nblocks(shape):
    _, o, m, band = shape
    return RC.plan_blocks(len(o), len(m), *band)[0]


def _run_on(rng, X, Y, d, xend, length=10):
    """Letters of two disjoint alphabets except one run of `length` matches on diagonal d whose last cell is (xend, xend - d)."""
    o = np.asarray((0, 1), np.uint8)[rng.integers(0, 2, X)]
    m = np.asarray((2, 3), np.uint8)[rng.integers(0, 2, Y)]
    yend = xend - d
    m[yend - length:yend] = o[xend - length:xend]
    return o, m


def cases():
    """[((id, origin, mutant, band), matrix, go, ge)] -- banded tables (B_LOCAL)."""
    rng = np.random.default_rng(161616)
    c2 = (cfg2_matrix(), CFG2[2], CFG2[3])
    out = []
    for d in (0, 1, 4, 5):
        for xend in (30, 31):
            o, m = _run_on(rng, 60, 58, d, xend)
            out.append((('run-d%d-x%d' % (d, xend), o, m, (-8, 7)),) + c2)
    o, m = _run_on(rng, 60, 58, 0, 30)
    out.append((('gaps-kept', o, m, (-8, 7)), gaps_matrix(), GAPS[2], GAPS[3]))
    for d in (0, 2):
        o, m = np.zeros(20, np.uint8), np.full(20, 2, np.uint8)                         # one match: cell (d + 1, 1)
        o[d] = m[0] = 1
        out.append((('first-d%d' % d, o, m, (-8, 7)),) + c2)
    for X in (40, 41):
        for Y in (40, 41):
            o, m = _run_on(rng, X, Y, X - Y, X)
            out.append((('last-%dx%d' % (X, Y), o, m, (-8, 7)),) + c2)
    out.append((('all-A', np.zeros(40, np.uint8), np.zeros(37, np.uint8), (-8, 7)),) + c2)
    by = {s[0]: s for s in SC.shapes()}
    out.append((by['disjoint'],) + c2)
    out.append((SC.top_shape(), SC.top_matrix(), -5., -2.))
    for n in (31, 39, 47, 55):                                                          # 4, 5, 6, 7 blocks
        o, m = _run_on(rng, n, n, 0, n)
        out.append((('blocks%d-late-rise' % ((2 * n + 1 + 15) // 16), o, m, (-5, 5)),) + c2)
    out.append((by['short'],) + c2)
    out.append((by['400x390-r20'],) + c2)
    out.append((by['400x390-r200'],) + c2)
    o = RC._rand(rng, 150)
    m = np.delete(RC._mutate(rng, o), [20, 21, 77, 130, 131, 132, 133, 134, 135, 136])
    out.append((('mixed-150x140', o, m, (-30, 30)), mixed_matrix(), -5., -2.))
    return out
