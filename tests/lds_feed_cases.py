"""Shapes shared by the tests of the letter rings (pw_wave.h, WaveFill16, LDSF; pw_plan.h, lds_feed): the packed kernel of rule
3 in matrix form, 8 diagonals per lane, one pair per wavefront, reads the matrix row of every origin letter and the selector
dword of every mutant letter from two rings of 512 letters in LDS, restaged 64 letters at a time once per 8 blocks.

What can go wrong there, and the smallest shape for each:
  * letters outside a sequence (the all-zero row, the "outside" selector) at both ends of either sequence, with sequences
    shorter than a chunk, a window, a dword: 1 .. 17 letters;
  * the first letter a lane reads at every residue mod 4 of its ring slot (the slot's row): bands that begin at diagonals
    -2, -4, -6, -8 (and the odd ones between them);
  * one sequence far shorter than the other: 400 x 24 and 24 x 400;
  * config 2's table shape, 400 x 390, at band radius 20 and 200;
  * the last section holds fewer than 8 blocks, and no block at all: block counts 0 .. 7 (mod 8);
  * the rings wrap: 1200 x 1190 at radius 200 runs 150 blocks, 1200 letters through rings of 512 -- more than twice round;
  * a mutant that ends in the middle of a chunk of 64 letters while the origin goes on.
"""
import numpy as np

from tests import ramp_free_cases as RC

CFG2 = ('cfg2', 1, -3, -5, -2)                 # (id, match, mismatch, go, ge)


def cfg2_matrix():
    return RC.matrix(CFG2[1], CFG2[2])


def nblocks(shape):
    _, o, m, band = shape
    return RC.plan_blocks(len(o), len(m), *band)[0]


def feed_residues(shape):
    """(e mod 4, f mod 4) of a shape: e, f are x and y of the band's lowest diagonal on step 0 (WaveFill16::run)."""
    _, o, m, band = shape
    dmin, dmax = max(band[0], -len(m)), min(band[1], len(o))
    amin = dmin if dmin > 0 else (-dmax if dmax < 0 else 0)
    s0 = amin - (amin - dmin) % 2
    return ((s0 + dmin) >> 1) % 4, ((s0 - dmin) >> 1) % 4


def shapes():
    """[(id, origin, mutant, band)] for the scores CFG2 -- banded tables (B_LOCAL)."""
    rng = np.random.default_rng(90211)
    out = []
    for n in range(1, 18):                                                              # 1 .. 17 letters
        o = RC._rand(rng, n)
        m = RC._mutate(rng, o) if n % 3 else np.concatenate([o[1:], RC._rand(rng, 2)])
        out.append(('len%d' % n, o, m, (-4, 4)))
    o = RC._rand(rng, 90)
    m = np.delete(RC._mutate(rng, o), [11, 40, 41])
    for dmin in range(-1, -9, -1):                                                      # every residue of e and f
        out.append(('dmin%d' % dmin, o, m, (dmin, 7)))
    l = RC._rand(rng, 400)
    out.append(('400x24', l, RC._mutate(rng, l[200:224], 0.1), (-24, 400)))
    out.append(('24x400', RC._mutate(rng, l[310:334], 0.1), l, (-400, 24)))
    _, o, m, _ = RC.bulk()[5]
    out.append(('400x390-r20', o, m, (-20, 20)))
    out.append(('400x390-r200', o, m, (-200, 200)))
    for nb in range(8, 16):                                                             # 8 .. 15 blocks: 0 .. 7 (mod 8)
        n = 8 * nb - 4                                                                  # 2 n + 1 steps
        o = RC._rand(rng, n)
        out.append(('blocks%d' % nb, o, RC._mutate(rng, o), (-5, 5)))
    o = RC._rand(rng, 300)
    out.append(('mutant-ends-mid-chunk', o, RC._mutate(rng, o)[:100], (-40, 220)))
    return out


def long_shape():
    """1200 x 1190 at radius 200: the rings wrap more than twice."""
    rng = np.random.default_rng(1200)
    o = RC._rand(rng, 1200)
    m = np.delete(RC._mutate(rng, o, 0.1), rng.choice(1200, 10, replace=False))
    return ('1200x1190-r200', o, m, (-200, 200))
