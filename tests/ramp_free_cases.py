"""Score sets, shapes and block arithmetic shared by the ramp_free tests (pw_plan.h, ramp_free: the packed matrix form of
the local rules runs the blocks in which diagonals start or end on its steady body where the scores allow it).

The predicate and the planner's block ranges are restated here from their definitions, not read from the code under
test; tests/test_ramp_free_plan.py holds the restated predicate against ``plan_only`` and tests/test_emu_ramp_free.py the
restated block ranges against the emulator's block counters.
"""
import numpy as np

B_LOCAL, LOCAL = 1, 1


def ramp_free(subst_min, go, ge):
    """On the integer scores the kernels hold: ge < 0, ge + go < 0, min(subst) < 0."""
    return ge < 0 and ge + go < 0 and subst_min < 0


def plan_blocks(X, Y, dmin, dmax):
    """(nblocks, steady_b0, steady_b1) of a banded table: block b (steps 16 b .. 16 b + 15, step t = x + y - s0) is steady
    iff every in-band diagonal holds its first cell before step 16 b and none has ended before step 16 b + 15."""
    dmin, dmax = max(dmin, -Y), min(dmax, X)
    amin = dmin if dmin > 0 else (-dmax if dmax < 0 else 0)
    s0 = amin - (amin - dmin) % 2
    first = [abs(d) - s0 for d in range(dmin, dmax + 1)]
    last = [abs(d) + 2 * (min(d, 0) + min(X - d, Y)) - s0 for d in range(dmin, dmax + 1)]
    nblocks = (max(last) + 1 + 15) // 16
    b0 = max(first) // 16 + 1
    b1 = min((min(last) + 1) // 16, nblocks)
    return nblocks, b0, max(b1, b0)


def block_kinds(X, Y, dmin, dmax):
    """Blocks the four loops of WaveFill16::run() take without ramp_free: [steady, not started, ended, both]."""
    nb, b0, b1 = plan_blocks(X, Y, dmin, dmax)
    lo, hi = min(b0, nb), min(b1, nb)
    counts = [hi - lo, 0, nb - hi, 0]
    counts[1 if b1 > b0 else 3] = lo
    return counts


def matrix(match, mismatch):
    return [[float(match if i == j else mismatch) for j in range(4)] for i in range(4)]


# ---- score sets: (id, match or None = the largest the shape admits, mismatch, go, ge) ----
SCORE_SETS = [('cfg2', 1, -3, -5, -2), ('go0', 1, -3, 0, -2), ('ge1-go0', 2, -2, 0, -1), ('min1-maxmatch', None, -1, -3, -2),
              ('ge100', 1, -3, 0, -100)]
# one step past each bound of the predicate: the planner refuses ramp_free and still names a packed kernel
REFUSED_SETS = [('ge0', 1, -3, -5, 0), ('ge0-go0', 1, -3, 0, 0), ('min0', 1, 0, -5, -2)]


def match_of(sset, x4, X, Y):
    """`None`: the largest match score admit_packed / packed_matrix_bytes_ok take for the shape -- max - min <= 127 (31
    times 4), every score within 100, min(X, Y) * max <= 8000 (2047 times 4)."""
    if sset[1] is not None:
        return sset[1]
    n = max(1, min(X, Y))
    return max(1, min((31 if x4 else 100) + sset[2], (2047 if x4 else 8000) // n))


def _rand(rng, n, letters=(0, 1, 2, 3)):
    return np.asarray(letters, np.uint8)[rng.integers(0, len(letters), n)]


def _mutate(rng, o, rate=0.15):
    m = o.copy()
    flip = rng.random(len(m)) < rate
    m[flip] = rng.integers(0, 4, int(flip.sum()))
    return m


def bulk(n=64):
    """n related pairs of 400 x 390, band radius 40."""
    rng = np.random.default_rng(77)
    out = []
    for _ in range(n):
        o = rng.integers(0, 4, 400).astype(np.uint8)
        m = o.copy()
        flip = rng.random(400) < 0.12
        m[flip] = rng.integers(0, 4, int(flip.sum()))
        out.append(('bulk', o, np.delete(m, rng.choice(400, 10, replace=False)), (-40, 40)))
    return out


def shapes():
    """[(id, origin, mutant, band)] -- banded tables (B_LOCAL)."""
    rng = np.random.default_rng(20261)
    out = []
    o = _rand(rng, 5)
    out.append(('short', o, np.concatenate([o, _rand(rng, 1)]), (-3, 3)))                      # 12 steps: less than a block
    o = _rand(rng, 150)
    out.append(('X<<Y', o[60:72].copy(), _mutate(rng, o), (-150, 12)))
    out.append(('X>>Y', _mutate(rng, o), o[31:44].copy(), (-12, 150)))
    # the outermost diagonals hold their first cell 1600 steps after the band's first
    l = _rand(rng, 1700)
    s = _mutate(rng, l[1500:1560], 0.1)
    out.append(('wait1600', l, s, (-1, 1600)))
    o = _rand(rng, 40)
    out.append(('band>table', o, _mutate(rng, o)[:33], (-500, 500)))
    out.append(('disjoint', _rand(rng, 50, (0, 1)), _rand(rng, 45, (2, 3)), (-10, 10)))      # best 0: the first cell
    core = _rand(rng, 20, (2, 3))
    out.append(('last-row', np.concatenate([_rand(rng, 30, (0, 1)), core]), np.concatenate([core, _rand(rng, 25, (0, 1))]), (-30, 30)))
    out.append(('last-col', np.concatenate([core, _rand(rng, 25, (0, 1))]), np.concatenate([_rand(rng, 30, (0, 1)), core]), (-30, 30)))
    o = _rand(rng, 47)
    out.append(('identical', o, o.copy(), (-5, 5)))                                          # best: the corner cell
    o = _rand(rng, 40)
    out.append(('mid-block', o, np.delete(_mutate(rng, o), [7, 19, 30]), (-6, 6)))             # 78 steps: 4 blocks and 14 steps
    # pairs whose best lies near the table's end, where a cell beyond a diagonal's end that read the sequence's last letters
    # again instead of letters outside it would outscore the table (three of the 64 pairs of the GPU test's batches)
    for k in (35, 36, 61):
        _, o, m, band = bulk()[k]
        out.append(('bulk%d' % k, o, m, band))
    return out
