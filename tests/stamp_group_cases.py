"""Shapes shared by the stamp-group tests (pw_wave.h, WaveFill16, GRP; pw_plan.h, stamp_group): the packed kernel of rule 3
in matrix form, 8 diagonals per lane, one pair per wavefront, keeps its running best as a key 8 (4 score) + (31 - cell within
a GROUP of four blocks) and stamps where the best was first reached once per group.

What can go wrong there, and the smallest shape for each:
  * the last group of a pair holds fewer than four blocks and is stamped behind the loop: block counts 0 .. 3 (mod 4), one
    pair shorter than a block;
  * an equal best in a later block or a later group of the same diagonal must lose: a periodic pair whose best recurs every
    18 cells of the main diagonal over 400 letters -- and the same pair with its LAST run one longer, so that the best rises
    in the final, partial group;
  * the position code: a best first reached in cell 0 and in cell 31 of a group;
  * no stamp at all: a pair without a match (best 0: every diagonal reports its first cell);
  * the key's top: best score 2047, key 65535 at position code 31;
  * config 2's table shape, 400 x 390, at band radius 20 and 200.
"""
import numpy as np

from tests import ramp_free_cases as RC

CFG2 = ('cfg2', 1, -3, -5, -2)                 # (id, match, mismatch, go, ge)


def cfg2_matrix():
    return RC.matrix(CFG2[1], CFG2[2])


def top_matrix():
    """Range 31 (the most the scores-times-4 bytes take), match 23: 89 matches reach 2047."""
    S = [[-8.0] * 4 for _ in range(4)]
    for i in range(4):
        S[i][i] = 23.0
    S[0][2] = S[2][0] = 3.0
    return S


def _runs(rng, lengths, gap=6):
    """Origin and mutant of equal length: runs of matches of the given lengths, `gap` mismatches behind each."""
    n = sum(lengths) + gap * len(lengths)
    o = rng.integers(0, 4, n).astype(np.uint8)
    m = o.copy()
    pos = 0
    for l in lengths:
        pos += l
        m[pos:pos + gap] = (o[pos:pos + gap] + 1 + rng.integers(0, 3, gap)) % 4
        pos += gap
    return o, m


def _single_run(rng, n, end, length=10):
    """Letters of two disjoint alphabets except one run of `length` matches whose last cell on the main diagonal is `end`."""
    o = np.asarray((0, 1), np.uint8)[rng.integers(0, 2, n)]
    m = np.asarray((2, 3), np.uint8)[rng.integers(0, 2, n)]
    m[end - length:end] = o[end - length:end]
    return o, m


def shapes():
    """[(id, origin, mutant, band)] for the scores CFG2 -- banded tables (B_LOCAL)."""
    rng = np.random.default_rng(4131)
    out = []
    o = RC._rand(rng, 5)
    out.append(('short', o, np.concatenate([o, RC._rand(rng, 1)]), (-3, 3)))            # 12 steps: one block, not a full one
    for n in (31, 39, 47, 55):                                                          # 4, 5, 6, 7 blocks
        o = RC._rand(rng, n)
        out.append(('blocks%d' % ((2 * n + 1 + 15) // 16), o, RC._mutate(rng, o), (-5, 5)))
    o, m = _runs(rng, [12] * 22)                                                        # 396 letters
    pad = 400 - len(o)
    out.append(('periodic', np.concatenate([o, np.zeros(pad, np.uint8)]), np.concatenate([m, np.full(pad, 1, np.uint8)]), (-20, 20)))
    o, m = _runs(rng, [12] * 21 + [13])                                                 # 397 letters: the last run rises to 13
    pad = 400 - len(o)
    out.append(('periodic-late-rise', np.concatenate([o, np.zeros(pad, np.uint8)]), np.concatenate([m, np.full(pad, 1, np.uint8)]),
                (-20, 20)))
    o, m = _single_run(rng, 120, 64)
    out.append(('cell0', o, m, (-8, 8)))
    o, m = _single_run(rng, 120, 95)
    out.append(('cell31', o, m, (-8, 8)))
    out.append(('disjoint', RC._rand(rng, 50, (0, 1)), RC._rand(rng, 45, (2, 3)), (-10, 10)))
    _, o, m, _ = RC.bulk()[5]
    out.append(('400x390-r20', o, m, (-20, 20)))
    out.append(('400x390-r200', o, m, (-200, 200)))
    return out


def top_shape():
    """(id, origin, mutant, band) for top_matrix(), go -5, ge -2: an exact copy of 89 letters -- best score 2047."""
    rng = np.random.default_rng(7189)
    o = rng.integers(0, 4, 400).astype(np.uint8)
    return ('best2047', o, o[3:92].copy(), (-200, 200))


def nblocks(shape):
    _, o, m, band = shape
    return RC.plan_blocks(len(o), len(m), *band)[0]
