"""Named inputs for the N-way seed index (kernels K9 of pw_mseeds.hip), each from a fixed RNG seed and each built to
land in one class of behaviour: every sequence count, unequal mixed radices, k-mers that fill whole 2048-row windows,
pairs that miss the neighbourhood by one on exactly one coordinate, pairs on which float and exact arithmetic
disagree, a long scrambled chain, and batches of hyper-boxes around the 64-box chunk.  tests/test_mseeds_cases.py
proves from the dense oracle alone (oracle/mseeds_dense_oracle.py) that every case lands where it is meant to;
tests/test_gpu_mseeds_every_n.py runs the same inputs on the device.

A case is a dict: ``seqs`` (uint8 arrays of letter indices), ``wordlen``, ``L`` (alphabet length) and what the case is
about.  Rows of the oracle are cached per case, computed once and never written to.

Two kinds of input:
  * *related sets* over ACGT: one shared core at random offsets, point-mutated at a rate that falls with N (a k-mer
    must survive in all N sequences to give a row);
  * *planted sets* over 36 letters: words over the letters 0 .. 3 between random spacers, the spacers of sequence s drawn
    from its own two letters 4 + 2 s and 5 + 2 s.  A k-mer that touches a spacer occurs in one sequence only, so the
    shared k-mers are exactly the planted words and their run lengths (the radices of the row decode) are the planted
    multiplicities -- which is what lets a k-mer be placed on a chosen row.
"""
from functools import lru_cache

import numpy as np

from oracle import mseeds_dense_oracle as DO

ALL_N = tuple(range(2, 17))
PLANT_L, PLANT_W = 36, 5            # 36 ** 5 < 2 ** 32: 4-byte keys; 16 sequences need 4 + 32 letters
EXP_ROWS = 2048                      # rows per workgroup of k_mexpand (kExpRows)
BOX_CHUNK = 64                       # boxes per blockIdx.y of k_mcount (kBoxChunk)
MAX_BOXES = BOX_CHUNK * 65535
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def case(seqs, wordlen, L, **kw):
    out = dict(seqs=[np.asarray(s, np.uint8) for s in seqs], wordlen=wordlen, L=L)
    out.update(kw)
    return out


_ROWS = {}


def rows_of(c):
    """The dense oracle's rows of a case (cached by the case's name; read-only)."""
    key = c['name']
    if key not in _ROWS:
        r = DO.seed_rows(c['seqs'], c['wordlen'], c['L'])
        r.setflags(write=False)
        _ROWS[key] = r
    return _ROWS[key]


# ---- every N ---------------------------------------------------------------------------------------------
EVERY_N_W = 8
EVERY_N_RADII = (8, 40)              # (d_radius, a_radius) of the graph on these sets


# 9014 draws a core with a repeated word: 2 ** 14 rows on top of the rest, past the 3000 this class is held to
EVERY_N_SEED = {14: 9114}


def mutation_rate(N):
    """Point mutations per letter: a word of 8 letters survives in all N copies with probability
    (1 - r) ** (8 N) ~ exp(-0.64), whatever N."""
    return .08 / N


@lru_cache(None)
def every_n(N):
    rng = np.random.default_rng(EVERY_N_SEED.get(N, 9000 + N))
    hom = int(rng.integers(150, 201))
    core = rng.integers(0, 4, hom)
    seqs = []
    for _ in range(N):
        c = core.copy()
        flip = rng.random(hom) < mutation_rate(N)
        c[flip] = (c[flip] + rng.integers(1, 4, int(flip.sum()))) % 4
        seqs.append(np.r_[rng.integers(0, 4, int(rng.integers(0, 120))), c, rng.integers(0, 4, int(rng.integers(0, 120)))])
    return case(seqs, EVERY_N_W, 4, name='every_n_%d' % N, N=N, core=hom)


@lru_cache(None)
def with_an_empty_member(N=5):
    c = every_n(N)
    seqs = list(c['seqs'])
    seqs[2] = np.zeros(0, np.uint8)
    return case(seqs, EVERY_N_W, 4, name='empty_member_%d' % N, N=N)


@lru_cache(None)
def with_a_member_one_short_of_a_word(N=5):
    c = every_n(N)
    seqs = list(c['seqs'])
    seqs[N - 1] = seqs[N - 1][:EVERY_N_W - 1]
    return case(seqs, EVERY_N_W, 4, name='short_member_%d' % N, N=N)


# ---- planted sets ----------------------------------------------------------------------------------------
def word(j):
    """The j-th planted word: PLANT_W letters over 0 .. 3, ascending with j as k-mer values."""
    assert 0 <= j < 4 ** PLANT_W
    return [(j >> (2 * (PLANT_W - 1 - t))) & 3 for t in range(PLANT_W)]


def plant(rng, N, plan):
    """plan[s]: list of word numbers and ('gap', n) entries, in sequence order.  Two words with no gap entry between
    them are separated by 1 .. 3 random spacer letters, as is the first word from the start; a gap entry gives
    exactly n."""
    seqs = []
    for s in range(N):
        spacer = lambda n: rng.integers(4 + 2 * s, 6 + 2 * s, n).tolist()     # noqa: E731
        out, gapped = [], False
        for item in plan[s]:
            if isinstance(item, tuple):
                out += spacer(item[1])
                gapped = True
                continue
            if not gapped:
                out += spacer(int(rng.integers(1, 4)))
            out += word(item)
            gapped = False
        seqs.append(out + spacer(int(rng.integers(1, 4))))
    return seqs


def plan_from_runs(rng, N, runs):
    """runs: {word number: (multiplicity in sequence 0, .., N - 1)} -> a plan with every sequence's words shuffled."""
    plan = []
    for s in range(N):
        items = [j for j, rl in runs.items() for _ in range(rl[s])]
        rng.shuffle(items)
        plan.append(items)
    return plan


# unequal radices: neighbours differ everywhere and at least three values occur; the product stays small
UNEQUAL = {3: (1, 2, 3), 7: (1, 2, 3, 1, 4, 1, 2), 11: (1, 2, 3, 1, 4, 1, 2, 1, 3, 1, 2),
           16: (1, 2, 1, 3, 1, 2, 1, 4, 1, 2, 1, 3, 1, 2, 1, 2)}
MIXED_N = (3, 7, 11, 16)


@lru_cache(None)
def mixed_radix(N):
    """Word 100: pairwise unequal radices with a 1 at s = 0 and 1s between larger ones; word 200: the same reversed, a 1
    at s = N - 1; word 300: 2 everywhere but a single 1 in the middle; words 400 ..: one hit in every sequence."""
    rng = np.random.default_rng(9100 + N)
    mid = tuple(1 if s == N // 2 else 2 for s in range(N)) if N <= 11 else \
        tuple(2 if s in (N // 2 - 1, N // 2 + 1) else 1 for s in range(N))
    runs = {100: UNEQUAL[N], 200: UNEQUAL[N][::-1], 300: mid}
    for j in range(400, 430):
        runs[j] = (1,) * N
    return case(plant(rng, N, plan_from_runs(rng, N, runs)), PLANT_W, PLANT_L, name='mixed_radix_%d' % N, N=N, runs=runs)


def _pad_runs(N, total, first):
    """Run-length tuples of words first, first + 1, .. whose products sum to `total`: two equal radices a at sequences that
    move with the word, 1 elsewhere (a radix of 1 between larger ones, at every position)."""
    runs, j = {}, first
    while total > 0:
        a = min(int(np.sqrt(total)), 40)
        rl = [1] * N
        rl[j % N] = a
        rl[(j + N // 2) % N] = a if N > 2 else 1
        runs[j] = tuple(rl)
        total -= int(np.prod(rl))
        j += 1
    assert total == 0
    return runs


# a k-mer of more than 4096 rows and one of more than 2048, per N (products of the radices)
BIG_RUNS = {3: ((17, 16, 16), (13, 13, 13)), 7: ((4, 3, 4, 3, 4, 3, 4), (3,) * 7),
            11: ((3, 3) + (2,) * 9, (3,) + (2,) * 10),
            16: ((2,) * 6 + (1,) + (2,) * 7 + (1, 1), (1, 2, 2, 1) + (2,) * 5 + (1,) + (2,) * 5 + (1,))}
WINDOW_STARTS = (EXP_ROWS - 1, EXP_ROWS, EXP_ROWS + 1)


@lru_cache(None)
def windows(N, start):
    """Padding words (numbers 1 ..) worth exactly `start` rows, then word 600 with more than 4096 rows -- it starts on row
    `start` and fills at least one whole workgroup window -- then word 700 with more than 2048."""
    rng = np.random.default_rng(9200 + 16 * N + start % 16)
    runs = _pad_runs(N, start, 1)
    runs[600], runs[700] = BIG_RUNS[N]
    return case(plant(rng, N, plan_from_runs(rng, N, runs)), PLANT_W, PLANT_L, name='windows_%d_%d' % (N, start), N=N,
                start=start, runs=runs)


@lru_cache(None)
def radix_two_everywhere():
    """N = 16, one k-mer twice in every sequence: 2 ** 16 rows, every radix 2.  Rows and box counts only."""
    rng = np.random.default_rng(9300)
    runs = {500: (2,) * 16, 501: (1,) * 16}
    return case(plant(rng, 16, plan_from_runs(rng, 16, runs)), PLANT_W, PLANT_L, name='radix_two_16', N=16, runs=runs)


# ---- near misses, one coordinate at a time ---------------------------------------------------------------------
NEAR_D, NEAR_A = 7, 30               # d_radius, a_radius: c = 30 / 7 is inexact in binary
NEAR_N = (3, 4, 9, 16)


def lands(d, delta, c, R):
    """Whether seeds whose d_k are d and d - delta pass the float test on that coordinate."""
    return bool(np.abs(np.float64(d) * np.float64(c) - np.float64(d - delta) * np.float64(c)) <= np.float64(R))


@lru_cache(None)
def near_miss(N, delta):
    """Word k (k = 1 .. N - 1) stands once in every sequence and a second time, `delta` letters on, in sequence k (counted
    from 0): its two seeds differ by `delta` in d_k and in a, and in nothing else.  delta = NEAR_D is inside the
    neighbourhood, NEAR_D + 1 outside.  Words stand 400 letters apart, far outside every radius, and each sequence's
    lead-in is chosen so that d_k c lands on the side of R that the exact product is on (c is inexact: for some d it
    does not, which is what the rounding cases are for)."""
    rng = np.random.default_rng(9400 + 16 * N + delta)
    c = 1. * NEAR_A / NEAR_D
    lead0, stride = 60, 400
    plan = []
    for s in range(N):
        lead = lead0 if s == 0 else next(
            x for x in range(int(rng.integers(1, 20)), lead0)
            if lands(lead0 - x, NEAR_D, c, NEAR_A) and not lands(lead0 - x, NEAR_D + 1, c, NEAR_A))
        items = [('gap', lead)]               # word 1 stands at `lead`, word k at lead + (k - 1) stride
        for k in range(1, N):
            items.append(k)
            used = PLANT_W
            if k == s:
                items += [('gap', delta - PLANT_W), k]
                used += delta
            items.append(('gap', stride - used))
        plan.append(items)
    fixed = plant(rng, N, plan)
    return case(fixed, PLANT_W, PLANT_L, name='near_miss_%d_%d' % (N, delta), N=N, delta=delta,
                d_radius=NEAR_D, a_radius=NEAR_A)


A_AXIS_T = 9
A_AXIS_N = (3, 4, 9, 16)


@lru_cache(None)
def a_axis(N):
    """One word twice in every sequence, A_AXIS_T letters apart: 2 ** N rows, of which the all-first and the all-second
    seed share every d and differ in a by N t.  With d_coeff = N t any other pair differs by at least t N t > N t on some
    d, so the only edge that radius N t allows beyond equal rows is that one -- and radius N t - 1 allows none."""
    rng = np.random.default_rng(9500 + N)
    plan = [[('gap', int(rng.integers(1, 30))), 1, ('gap', A_AXIS_T - PLANT_W), 1] for _ in range(N)]
    return case(plant(rng, N, plan), PLANT_W, PLANT_L, name='a_axis_%d' % N, N=N, t=A_AXIS_T, radius=N * A_AXIS_T)


# ---- rounding ------------------------------------------------------------------------------------------------
ROUND_C, ROUND_R, ROUND_DELTA = .1, .3, 3


@lru_cache(None)
def rounding(axis, d0):
    """N = 3 over ACGT, word AAAAA.  Sequence `axis` (1 or 2) holds a run of 7 As, the other two runs of 6: the word stands
    at 3 consecutive places there and at 2 in the others.  Among the 12 rows are pairs with equal a that differ by 3 in
    d_axis alone ((i, j + 2, l) and (i + 1, j, l + 1) for axis 1), at d_axis = d0 + 2 and d0 - 1."""
    assert axis in (1, 2)
    w = 5
    lead = [40, 40, 40]
    lead[axis] = 39 - d0
    seqs = []
    for s in range(3):
        other = [1, 2, 3][s]                    # C, G or T: no second word is shared
        seqs.append([other] * lead[s] + [0] * (w + (2 if s == axis else 1)) + [other] * 3)
    return case(seqs, w, 4, name='rounding_%d_%d' % (axis, d0), N=3, axis=axis, d0=d0)


# d0 = 1: d_axis 3 against 0, fl(.1 * 3) - 0 > .3, where 3 / 10 <= 3 / 10 in decimal; d0 = 7: 9 against 6,
# fl(.1 * 9) - fl(.1 * 6) < .3 although the doubles .1 and .3 satisfy 3 * .1 > .3 exactly
ROUNDING_D0 = (1, 7)
# the other direction, (c, R, d0): d_axis 7 against 4, 3 * .3 <= .9 on the doubles themselves, fl(.3 * 7) - fl(.3 * 4) > .9
ROUNDING_OTHER_WAY = (.3, .9, 5)


# ---- chains --------------------------------------------------------------------------------------------------
CHAIN_LEN, CHAIN_W = 3000, 12
CHAIN_RADII = (4, 7)                 # |a - a'| <= R with a = 3 i: one hop either way, two hops either way


@lru_cache(None)
def chain():
    """Three copies of one random sequence with no repeated 12-mer: row i-th-k-mer = (0, 0, 3 i), a single diagonal
    chain whose rows come in k-mer order, that is scrambled along the chain."""
    rng = np.random.default_rng(9600)
    s = rng.integers(0, 4, CHAIN_LEN)
    return case([s, s.copy(), s.copy()], CHAIN_W, 4, name='chain', N=3)


def chain_masks(n):
    rng = np.random.default_rng(9601)
    every50 = np.ones(n, bool)
    every50[::50] = False
    return {'all': np.ones(n, bool), 'none': np.zeros(n, bool), 'every_50th_off': every50, 'random_half': rng.random(n) < .5}


# ---- boxes -----------------------------------------------------------------------------------------------------
BOX_BATCHES = (1, 63, 64, 65, 128, 129, 1000)


@lru_cache(None)
def many_rows():
    """N = 3, three unrelated sequences of 430 letters at word length 2: about 3 x 10^5 rows, more than the 1024 x 256
    that one pass of k_mcount's grid covers."""
    rng = np.random.default_rng(9700)
    return case([rng.integers(0, 4, 430) for _ in range(3)], 2, 4, name='many_rows', N=3)


def boxes(rows, n_boxes, seed):
    """(lo, hi, have) for n_boxes boxes; a smaller batch is a prefix of these.  The first 4 N + 6 are the named shapes, in this order: each coordinate bounded
    alone (N); lo == hi == an existing value per coordinate (N); lo > hi per coordinate (N); the whole int32 range
    per coordinate (N); nothing bounded; everything bounded to the int32 range; the bounding box of the rows; one row
    exactly; bounds (INT32_MIN, min - 1) and (max + 1, INT32_MAX).  The rest are random boxes around random rows."""
    rng = np.random.default_rng(seed)
    rows = np.asarray(rows, np.int64)
    N = rows.shape[1]
    lo, hi, have = np.zeros((n_boxes, N), np.int64), np.zeros((n_boxes, N), np.int64), np.zeros((n_boxes, N), np.uint8)
    assert n_boxes >= n_named_boxes(N)
    pick = rows[rng.integers(0, len(rows), n_boxes)] if len(rows) else np.zeros((n_boxes, N), np.int64)
    named = []
    for k in range(N):
        named.append({k: (pick[k, k] - 25, pick[k, k] + 25)})
    for k in range(N):
        named.append({k: (pick[k, k], pick[k, k])})
    for k in range(N):
        named.append({k: (pick[k, k] + 1, pick[k, k])})
    for k in range(N):
        named.append({k: (I32_MIN, I32_MAX)})
    named.append({})
    named.append({k: (I32_MIN, I32_MAX) for k in range(N)})
    mn = rows.min(0) if len(rows) else np.zeros(N, np.int64)
    mx = rows.max(0) if len(rows) else np.zeros(N, np.int64)
    named.append({k: (mn[k], mx[k]) for k in range(N)})
    named.append({k: (pick[0, k], pick[0, k]) for k in range(N)})
    named.append({0: (I32_MIN, mn[0] - 1)})
    named.append({N - 1: (mx[N - 1] + 1, I32_MAX)})
    for b in range(n_boxes):
        if b < len(named):
            spec = named[b]
        else:
            spec = {k: (pick[b, k] - int(rng.integers(0, 40)), pick[b, k] + int(rng.integers(0, 40)))
                    for k in range(N - 1) if rng.random() < .6}
            if rng.random() < .7:
                spec[N - 1] = (pick[b, N - 1] - int(rng.integers(0, 600)), pick[b, N - 1] + int(rng.integers(0, 600)))
        for k, (l, h) in spec.items():
            lo[b, k], hi[b, k], have[b, k] = l, h, 1
    return lo.astype(np.int32), hi.astype(np.int32), have


def n_named_boxes(N):
    return 4 * N + 6


def as_bands(lo, hi, have):
    """The (ds_band, a_band) form of seed_counts for the same boxes."""
    out = []
    for l, h, v in zip(lo.tolist(), hi.tolist(), have.tolist()):
        ds = [(l[k], h[k]) if v[k] else None for k in range(len(l) - 1)]
        out.append((ds, (l[-1], h[-1]) if v[-1] else None))
    return out


@lru_cache(None)
def tiny_pair():
    """N = 2, a handful of rows: the index under the largest box batch the C ABI admits."""
    return case([[0, 1, 2, 3, 0, 1, 2], [1, 2, 3, 0, 1, 3]], 3, 4, name='tiny_pair', N=2)


def max_boxes(rows):
    """MAX_BOXES boxes on a tiny index, built with whole-array numpy (box b depends on b alone)."""
    rows = np.asarray(rows, np.int64)
    N = rows.shape[1]
    b = np.arange(MAX_BOXES, dtype=np.int64)
    r = rows[b % len(rows)]
    lo = r - (b[:, None] // 7 + np.arange(N)) % 5
    hi = r + (b[:, None] // 3 + np.arange(N)) % 4 - (b[:, None] % 11 == 0)
    have = ((b[:, None] >> np.arange(N)) & 1 | (b[:, None] % 5 == 0)).astype(np.uint8)
    return lo.astype(np.int32), hi.astype(np.int32), have
