"""Named read pairs that pin which scoring path of biseqt_amd/csrc/pw_overlap.hip a pair takes, built from fixed RNG seeds
(no committed data), and the expected records from oracle/overlap_record_oracle.py.

The paths are selected by two numbers of a pair: its seed count (<= 64: one wavefront; 65 .. 2048: one workgroup from the
seed list on the all-pairs path; otherwise the per-diagonal histogram) and, in the histogram kernel, its number of occupied
diagonals (<= 1024: every score kept from pass 1; <= 8192: listed diagonals, scores above 1024 re-evaluated; more: every
thread walks its own chunk).  Every case carries the class it must land in (`klass`); tests/test_overlap_cases.py asserts
it on the CPU from the oracle alone, which is what proves that the GPU test reaches the path.

An exact seed count is a search: T and a mutated overlapping S; cum[i] = seeds of the first i k-mers of S against T is
non-decreasing; S is cut at the first prefix with cum == target, the next RNG seed is taken when no prefix hits it.
"""
import collections
import functools

import numpy as np

from oracle import overlap_record_oracle as RO
from tests import wide_words as WW

Case = collections.namedtuple('Case', 'name reads wordlen alphabet_len g_max sensitivity complement klass call')

COMPLEMENT = {
    4: np.array([3, 2, 1, 0], np.uint8),
    2: np.array([1, 0], np.uint8),                                                   # the swap
    20: np.array([1, 0, 3, 2, 5, 4, 7, 6, 9, 8, 11, 10, 13, 12, 15, 14, 17, 16, 18, 19], np.uint8),   # fixed points 18, 19
    3: np.array([2, 1, 0], np.uint8),                                                # fixed point 1
    36: np.arange(35, -1, -1).astype(np.uint8),                                      # the reversal: 32 .. 35 <-> 3 .. 0
}
SEED_TARGETS = (1, 2, 63, 64, 65, 66, 2047, 2048, 2049, 2050)
SMALL_MAX, MEDIUM_MAX, KEEP_MAX, LISTED_MAX = 64, 2048, 1024, 8192


def revcomp(x, alphabet_len):
    return COMPLEMENT[alphabet_len][np.asarray(x, np.uint8)[::-1]].astype(np.uint8)


def _u8(x):
    return np.ascontiguousarray(x, np.uint8)


def _rand(rng, L, n):
    return rng.integers(0, L, n).astype(np.uint8)


def _mutate(rng, x, L, rate):
    """Substitutions at `rate` and indels at `rate` (half deletions, half insertions)."""
    u = rng.random(len(x))
    sub = rng.random(len(x)) < rate
    new = rng.integers(0, L, len(x))
    ins = rng.integers(0, L, len(x))
    out = []
    for q, c in enumerate(x.tolist()):
        if u[q] < rate / 2:
            continue
        if u[q] < rate:
            out.append(int(ins[q]))
        out.append(int(new[q]) if sub[q] else c)
    return np.array(out, np.uint8)


def _exact_seeds(target, L, k, t_len, first_seed, stretch, min_nocc=0):
    """(S, T) with exactly `target` seeds: S is a prefix of a 2 % mutated copy of a stretch that overlaps T.  The targets of
    one tier share T (one read of an all-pairs union) and take S from stretches `stretch` = 0, 1, 2, ... that start an
    eighth of T apart and are mutated independently: reads that overlap each other, not prefixes of one read."""
    for seed in range(first_seed, first_seed + 50):
        rng = np.random.default_rng(seed)
        G = _rand(rng, L, 2 * t_len)
        T = G[:t_len].copy()
        start = (1 + stretch) * t_len // 8
        S = _mutate(np.random.default_rng([seed, target]), G[start: start + t_len], L, .02)
        kS, kT = RO.kmer_keys(S, k, L), np.sort(RO.kmer_keys(T, k, L))
        cum = np.cumsum(np.searchsorted(kT, kS, 'right') - np.searchsorted(kT, kS, 'left'))
        hit = np.flatnonzero(cum == target)
        if len(hit):
            S = S[:int(hit[0]) + k].copy()                # the first hit[0] + 1 k-mers of S
            if len(np.unique(RO.seed_diagonals(S, T, k, L))) >= min_nocc:
                return S, T
    raise AssertionError('no prefix with %d seeds' % target)


def _seed_class(target):
    return dict(seeds=target, nocc=(20, None)) if target >= 63 else dict(seeds=target)


def _first_with(make, pred, first_seed, what):
    for seed in range(first_seed, first_seed + 200):
        S, T, k, L, g, sens = make(np.random.default_rng(seed))
        if pred(record(S, T, k, L, g, sens)):
            return S, T
    raise AssertionError('no RNG seed gives ' + what)


@functools.lru_cache(maxsize=None)
def _record(s, t, k, L, g, sens):
    return RO.band_record(np.frombuffer(s, np.uint8), np.frombuffer(t, np.uint8), k, L, g, sens)


def record(S, T, k, L, g, sens):
    """The oracle record of (S, T), computed once per session and never modified."""
    return _record(_u8(S).tobytes(), _u8(T).tobytes(), int(k), int(L), float(g), float(sens))


def case_record(c, swapped=False):
    S, T = c.reads[::-1] if swapped else c.reads
    return record(S, T, c.wordlen, c.alphabet_len, c.g_max, c.sensitivity)


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, S, T, k, L, g, sens, call='', **klass):
        out.append(Case(name, (_u8(S), _u8(T)), k, L, g, sens, COMPLEMENT[L], klass, call))

    # ---- exact seed counts around the tier bounds 64 | 65 and 2048 | 2049 ----
    for L, k, t_len, params in ((4, 6, (5000, 2600), ((.2, .99), (.1, .9))), (20, 3, (6000, 3000), ((.3, .99), (.2, .9)))):
        for target in SEED_TARGETS:
            S, T = _exact_seeds(target, L, k, t_len[target > 66], 0, SEED_TARGETS.index(target) % 6, 20 if target >= 63 else 0)
            g, sens = params[target > 66]
            add('seeds%d_L%d' % (target, L), S, T, k, L, g, sens, **_seed_class(target))

    # ---- occupied diagonals around the bounds 1024 | 1025 and 8192 | 8193 of the histogram kernel ----
    rng = np.random.default_rng(101)
    S, T = (_rand(rng, 2, 500) for _ in range(2))                     # two of four letters: 16 x the seeds per diagonal
    add('dense_nocc_le_1024', S, T, 4, 4, .2, .99, seeds=(MEDIUM_MAX + 1, None), nocc=(1, KEEP_MAX))
    S, T = (_rand(rng, 4, 1500) for _ in range(2))
    add('dense_nocc_1025_8192', S, T, 4, 4, .2, .99, seeds=(MEDIUM_MAX + 1, None), nocc=(KEEP_MAX + 1, LISTED_MAX))
    S, T = (_rand(rng, 4, 4500) for _ in range(2))
    add('dense_nocc_gt_8192', S, T, 3, 4, .2, .99, seeds=(MEDIUM_MAX + 1, None), nocc=(LISTED_MAX + 1, None))
    add('short_vs_4500', _rand(rng, 4, 40), T, 3, 4, .2, .99, seeds=(MEDIUM_MAX + 1, None), nocc=(KEEP_MAX + 1, LISTED_MAX))   # the group's third read
    S, T = (_rand(rng, 4, 2800) for _ in range(2))                    # the pair-list path alone sends it to the dense kernel
    add('medium_nocc_gt_1024', S, T, 6, 4, .1, .9, seeds=(SMALL_MAX + 1, MEDIUM_MAX), nocc=(KEEP_MAX + 1, LISTED_MAX))

    # ---- table shapes: |S| + |T| + 1 counters, dealt to 256 threads in chunks ----
    for name, ls, lt in (('table_255', 127, 127), ('table_256', 127, 128), ('table_257', 128, 128), ('table_513', 300, 212)):
        S, T = _rand(rng, 4, ls), _rand(rng, 4, lt)
        add(name, S, T, 3, 4, .1, .99, seeds=(SMALL_MAX + 1, None), table=int(name[6:]))
    S, T = _rand(rng, 4, 30), _rand(rng, 4, 3000)
    add('unequal_30_3000', S, T, 3, 4, .1, .99, seeds=(SMALL_MAX + 1, MEDIUM_MAX), table=3031)
    T = _rand(rng, 4, 200)
    add('one_word', T[50:53].copy(), T, 3, 4, .1, .99, seeds=(1, None), s_len=3)
    add('empty_read', np.zeros(0, np.uint8), T, 3, 4, .1, .99, seeds=0)
    add('shorter_than_word', T[:2].copy(), T, 3, 4, .1, .99, seeds=0)

    # ---- corners: the only shared k-mer is the suffix of S and the prefix of T, d = |S| - k; and mirrored ----
    S = np.concatenate([_rand(rng, 2, 40), [2, 3, 2]])
    T = np.concatenate([[2, 3, 2], np.full(40, 3)])
    add('corner_suffix_prefix', S, T, 3, 4, .1, .99, seeds=1, d_best=len(S) - 3)
    add('corner_prefix_suffix', T, S, 3, 4, .1, .99, seeds=1, d_best=-(len(S) - 3))
    # the best diagonal within r of the table edge, so that its window [d - r, d + r] crosses the edge and is clamped: one
    # 2-mer in the very corner, d = -(|T| - 2) with L = 3 and r = 3 > k at g_max .3, sensitivity .99; and mirrored
    S = np.concatenate([[0, 2, 1], _rand(rng, 2, 30)])
    T = np.concatenate([2 + _rand(rng, 2, 30), [3, 0, 2]])
    add('clamp_at_minus_lenT', S, T, 2, 4, .3, .99, seeds=1, clamp='low')
    add('clamp_at_lenS', T, S, 2, 4, .3, .99, seeds=1, clamp='high')

    # the same in every seed-count tier: random reads that share a run of three equal letters in either corner of the
    # table, so the extreme diagonals d = |S| - 2 and d = -(|T| - 2) are occupied, their windows (r = 3) cross the edge and,
    # with the seeds of the run beside them, one of them is the best diagonal with w > 0 -- evaluated by the wavefront
    # kernel, the seed-list kernel and the three branches of the histogram kernel
    def cornered(ls, lt):
        S, T = _rand(rng, 4, ls), _rand(rng, 4, lt)
        S[-3:], T[:3], S[:3], T[-3:] = 0, 0, 3, 3
        return S, T
    for name, ls, lt, klass in (('clamp_small', 12, 12, dict(seeds=(2, SMALL_MAX))),
                                ('clamp_medium', 60, 60, dict(seeds=(SMALL_MAX + 1, MEDIUM_MAX))),
                                ('clamp_dense_nocc_le_1024', 300, 300, dict(seeds=(MEDIUM_MAX + 1, None), nocc=(20, KEEP_MAX))),
                                ('clamp_dense_nocc_1025_8192', 1000, 1000, dict(seeds=(MEDIUM_MAX + 1, None), nocc=(KEEP_MAX + 1, LISTED_MAX))),
                                ('clamp_dense_nocc_gt_8192', 300, 8300, dict(seeds=(MEDIUM_MAX + 1, None), nocc=(LISTED_MAX + 1, None),
                                                                             call='long'))):
        for _ in range(20):                             # (a chance diagonal can outscore the corners: draw again)
            S, T = cornered(ls, lt)
            o = record(S, T, 2, 4, .3, .99)
            if o['d_best'] - o['r_best'] < -lt or o['d_best'] + o['r_best'] > ls:
                break
        add(name, S, T, 2, 4, .3, .99, clamps='best', **klass)
    S = _rand(rng, 4, 40)                                # a third read for the call of the 8300-letter pair, as cornered
    S[-3:], S[:3] = 0, 3
    add('clamp_short_vs_8300', S, T, 2, 4, .3, .99, call='long', clamps='any', seeds=(MEDIUM_MAX + 1, None), nocc=(KEEP_MAX + 1, LISTED_MAX))

    # ---- non-positive scores: tie == nocc and the *_first fields decide ----
    add('w_zero', [0, 1, 2, 3] * 3 + [1], [1] + [3, 2, 0, 0] * 3, 1, 4, .2, .99, seeds=40, nocc=(18, 18), w_zero=True,
        first_differs=True)
    S, T = np.zeros(12, np.uint8), np.full(12, 3, np.uint8)
    S[[3, 9]], T[[7, 2]] = (1, 2), (1, 2)
    add('w_negative', S, T, 1, 4, .2, .99, seeds=2, nocc=(2, 2), w_negative=True)

    # two letters, wordlen 1: the blocks keep the corners of the table empty, every long diagonal scores below chance
    def blocks(c, mid):
        def make(r):
            return (np.concatenate([np.zeros(c), _rand(r, 2, mid), np.zeros(c)]),
                    np.concatenate([np.ones(c), _rand(r, 2, mid), np.ones(c)]), 1, 2, .3, .99)
        return make
    S, T = _first_with(blocks(40, 120), lambda o: o['n_seeds'] > MEDIUM_MAX and o['w_best'] < 0, 0, 'a dense pair with w_best < 0')
    add('w_negative_dense_L2', S, T, 1, 2, .3, .99, seeds=(MEDIUM_MAX + 1, None), nocc=(20, KEEP_MAX), w_negative=True)
    rng = np.random.default_rng(202)
    G = _rand(rng, 2, 400)
    add('overlap_L2', G[:300].copy(), _mutate(rng, G[100:], 2, .02), 9, 2, .2, .9, seeds=(SMALL_MAX + 1, MEDIUM_MAX), w_positive=True)
    add('sparse_L2', _rand(rng, 2, 60), _rand(rng, 2, 70), 9, 2, .2, .9, seeds=(1, SMALL_MAX))

    # ---- ties ----
    add('w_above_one_periodic', [0, 1, 2, 3] * 25, [0, 1, 2, 3] * 30, 6, 4, .2, .99, seeds=(MEDIUM_MAX + 1, None), w_ge_one=True, tie=(2, None))

    def doubled(r):
        U = _rand(r, 4, 50)
        return U, np.concatenate([U, U]), 6, 4, .2, .99
    S, T = _first_with(doubled, lambda o: o['tie'] >= 2 and 0 < o['w_best'] < 1, 0, 'two equal best diagonals')
    add('two_equal_best', S, T, 6, 4, .2, .99, seeds=(SMALL_MAX + 1, MEDIUM_MAX), tie=(2, None), w_positive=True, w_below_one=True)

    # A near tie: a block of 8 words on a diagonal with L = 30 and one of 16 words on a diagonal with L = 60, nothing else shared
    # (the fillers use disjoint letters).  (n + 1) / L is 4 / 15 on both, their radii differ and p0 = 4^-20, so the two w differ by
    # 7e-12 relative: within the tie rule's 1e-9 (tie = 2), yet not equal (a rule without the tolerance would say tie = 1).
    rng = np.random.default_rng(303)
    X, Y = _rand(rng, 4, 8 + 19), _rand(rng, 4, 16 + 19)
    S = np.concatenate([_rand(rng, 2, 10), Y, X])
    T = np.concatenate([X, 2 + _rand(rng, 2, 3), Y, 2 + _rand(rng, 2, 9)])
    add('near_tie', S, T, 20, 4, .2, .9, seeds=24, nocc=(2, 2), tie=(2, 2), near_tie=True, w_positive=True, w_below_one=True)

    # ---- long words: one group per key width, every case with the top and the zero word (tests/wide_words.py) ----
    for (L, k), (g, sens) in WW.OVERLAP_RUNGS.items():
        for x in WW.inputs(L, k).values():
            add('wide_L%d_k%d_%s' % (L, k, x.name), x.S, x.T, k, L, g, sens, **_wide_class(x))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def _wide_class(x):
    L, k = x.alphabet_len, x.wordlen
    kl = dict(mod32=True) if L ** k > 2 ** 33 and x.kind in ('basic', 'sparse', 'empty') else {}
    if x.kind != 'empty':
        kl['key_bits'] = WW.KEY_BITS[(L, k)]
    kl.update({'basic': dict(seeds=(SMALL_MAX + 1, MEDIUM_MAX), tie=(1, 1), w_positive=True, w_below_one=True),
               'sparse': dict(seeds=(1, SMALL_MAX)),
               'empty': dict(seeds=0),
               'periodic': dict(seeds=(MEDIUM_MAX + 1, 5000), nocc=(20, KEEP_MAX), tie=(2, None), w_ge_one=True),
               'doubled': dict(seeds=(SMALL_MAX + 1, MEDIUM_MAX), tie=(2, 2), w_positive=True, w_below_one=True)}[x.kind])
    return kl


def check_class(c):
    """Asserts, from the oracle alone, that the case lands in the class its name promises."""
    o, (S, T), kl = case_record(c), c.reads, dict(c.klass)

    def within(v, rng, what):
        lo, hi = rng if isinstance(rng, tuple) else (rng, rng)
        assert (lo is None or v >= lo) and (hi is None or v <= hi), '%s: %s = %d not in %r' % (c.name, what, v, rng)

    within(o['n_seeds'], kl.pop('seeds'), 'n_seeds')
    if 'nocc' in kl:
        within(o['nocc'], kl.pop('nocc'), 'nocc')
    if 'tie' in kl:
        within(o['tie'], kl.pop('tie'), 'tie')
    if 'table' in kl:
        assert len(S) + len(T) + 1 == kl.pop('table')
    if 's_len' in kl:
        assert len(S) == kl.pop('s_len') == c.wordlen
    if 'd_best' in kl:
        assert o['d_best'] == kl.pop('d_best') == o['d_first']
    if 'clamp' in kl:
        if kl.pop('clamp') == 'low':
            assert o['d_best'] - o['r_best'] < -len(T) < o['d_best']
        else:
            assert o['d_best'] + o['r_best'] > len(S) > o['d_best']
    if 'clamps' in kl:
        assert clamped(o, S, T) == (True, True) and o['w_best'] > 0
        if kl.pop('clamps') == 'best':                    # and the best diagonal is one of them
            assert o['d_best'] - o['r_best'] < -len(T) or o['d_best'] + o['r_best'] > len(S)
    if 'key_bits' in kl:                                  # the largest key uses every bit the join sorts on
        keys = np.concatenate([RO.kmer_keys(S, c.wordlen, c.alphabet_len), RO.kmer_keys(T, c.wordlen, c.alphabet_len)])
        assert int(keys.max()).bit_length() == kl.pop('key_bits') == (c.alphabet_len ** c.wordlen - 1).bit_length()
        assert int(keys.min()) == 0 and int(keys.max()) == c.alphabet_len ** c.wordlen - 1
    if kl.pop('mod32', False):                            # a join on the low 32 bits of the keys counts other seeds
        kS, kT = RO.kmer_keys(S, c.wordlen, c.alphabet_len), RO.kmer_keys(T, c.wordlen, c.alphabet_len)
        assert WW.count_seeds(kS, kT) == o['n_seeds'] != WW.count_seeds(kS & 0xffffffff, kT & 0xffffffff)
    if kl.pop('w_zero', False):
        assert o['w_best'] == 0.0 and o['tie'] == o['nocc'] > 1
    if kl.pop('w_negative', False):
        assert o['w_best'] < 0 and o['tie'] == o['nocc'] > 1
    if kl.pop('near_tie', False):                         # the tied scores are unequal, apart by less than the rule's 1e-9
        assert 0 < abs(o['w'][0] - o['w'][1]) < 1e-10 * o['w_best']
    if kl.pop('first_differs', False):
        assert o['d_first'] != o['d_best']
    if kl.pop('w_positive', False):
        assert o['w_best'] > 0
    if kl.pop('w_below_one', False):
        assert o['w_best'] < 1
    if kl.pop('w_ge_one', False):
        assert o['w_best'] >= 1
    assert not kl, kl
    assert 0 < c.g_max < 1 and c.g_max in (.1, .2, .3) and c.sensitivity in (.9, .99)
    comp = c.complement
    assert len(comp) == c.alphabet_len and (comp[comp] == np.arange(c.alphabet_len)).all()


def clamped(o, S, T):
    """Whether some occupied diagonal's window [d - r, d + r] crosses the low edge -|T| of the table, and some the high
    edge |S|: (low, high)."""
    return bool((o['d'] - o['r'] < -len(T)).any()), bool((o['d'] + o['r'] > len(S)).any())


def tier(o):
    """The scoring path a record's pair takes, by seed count and occupied diagonals."""
    if o['n_seeds'] <= MEDIUM_MAX:
        return 'small' if o['n_seeds'] <= SMALL_MAX else 'medium'
    return 'dense_kept' if o['nocc'] <= KEEP_MAX else 'dense_listed' if o['nocc'] <= LISTED_MAX else 'dense_chunks'


def groups():
    """Cases that share (alphabet_len, wordlen, g_max, sensitivity) and go into one call, in case order.  The pairs with more
    than 8192 occupied diagonals keep a call of three reads to themselves (`call`): the oracle takes most of a second for
    each pair with such a read."""
    out = collections.OrderedDict()
    for c in cases():
        out.setdefault((c.alphabet_len, c.wordlen, c.g_max, c.sensitivity, c.call), []).append(c)
    return out


def group_id(key):
    return 'L%d_k%d_g%g_s%g' % key[:4] + ('_' + key[4] if key[4] else '')


def interleaved(group):
    """The group's cases ordered so that sparse, dense and empty pairs alternate (by seed count: smallest, largest, second
    smallest, ...)."""
    by = sorted(group, key=lambda c: (case_record(c)['n_seeds'], c.name))
    out = []
    while by:
        out.append(by.pop(0))
        if by:
            out.append(by.pop())
    return out
