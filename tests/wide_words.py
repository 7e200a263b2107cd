"""Read pairs for long words: inputs that pin the three sort-merge joins (biseqt_amd/csrc/pw_seeds.hip, pw_mseeds.hip,
pw_overlap.hip) at every width of the k-mer key L^k, built from fixed RNG seeds (no committed data).

The joins change code path with the key: 4-byte keys while L^k < 0xffffffff and 8-byte keys from there on (pairwise and
N-way index), a sort on bits(L^k - 1) bits, and on the overlap pair-list path the key (pair << kbits) | k-mer, which cuts a
call into chunks of fewer than 2^(62 - kbits) pairs.  LADDER holds one (alphabet_len, wordlen) per width worth telling
apart; `inputs(L, k)` gives the pairs of a rung.  tests/test_wide_words.py asserts on the CPU, from the oracles alone, that
every input can tell a wrong join from a right one: the largest key uses every bit of the sort, keys 0 and L^k - 1 occur, a
k-mer has several hits on either side, words that differ in one end letter (or by 2^32 in the key) give no seed, and a join
on keys cut to 32 bits would count other seeds.
"""
import collections
import functools

import numpy as np

from oracle import overlap_record_oracle as RO

# (alphabet_len, wordlen): L^k = 2^30 | 2^31 | 3 486 784 401, the last below 0xffffffff | 2^32, the first 8-byte key (the
# word length of the 50 000-read workload) | 34 bits | 48 bits | 57 bits, letters >= 32 | 2^60 | 61 bits
LADDER = ((4, 15), (2, 31), (3, 20), (4, 16), (3, 21), (4, 24), (36, 11), (4, 30), (20, 14))
KEY_BITS = {(4, 15): 30, (2, 31): 31, (3, 20): 32, (4, 16): 32, (3, 21): 34, (4, 24): 48, (36, 11): 57, (4, 30): 60, (20, 14): 61}
KEY_TYPE = {(4, 15): 32, (2, 31): 32, (3, 20): 32, (4, 16): 64, (3, 21): 64, (4, 24): 64, (36, 11): 64, (4, 30): 64, (20, 14): 64}
# the rungs that go through the overlap record tests, with the (g_max, sensitivity) of their group
OVERLAP_RUNGS = collections.OrderedDict((((3, 20), (.1, .9)), ((4, 16), (.2, .99)), ((36, 11), (.3, .99)), ((4, 30), (.2, .9)),
                                         ((20, 14), (.1, .99))))
NWAY = ((3, 20, 3), (4, 16, 3), (4, 24, 3), (36, 11, 3), (4, 16, 5))      # (alphabet_len, wordlen, sequences) of the N-way index
EDGE = (4, 31)                                           # L^k = 2^62: the overlap entry points take it, the indices refuse it

Input = collections.namedtuple('Input', 'name kind S T alphabet_len wordlen planted')


def key_bits(L, k):
    """The width of the k-mer keys: the bits of L^k - 1 (pw_overlap.hip: check_args; pw_seeds_create without mask sets)."""
    return max(1, (L ** k - 1).bit_length())


def key_type(L, k):
    """The documented rule of pw_seeds_create and pw_mseeds_create: 4-byte keys while L^k < 0xffffffff."""
    return 32 if L ** k < 0xffffffff else 64


def pairs_per_chunk(L, k):
    """The most pairs of one chunk of a pair-list call, where the key width bounds it (pw_overlap.hip: bands): a chunk holds
    fewer than 2^(62 - kbits) pairs and at least one; None where 62 - kbits >= 40 (only the sizes bound a chunk)."""
    bits = 62 - key_bits(L, k)
    return None if bits >= 40 else max(1, 2 ** bits - 1)


def chunk_sizes(n_pairs, L, k):
    """The chunks a pair-list call of n_pairs short pairs is cut into."""
    per = pairs_per_chunk(L, k) or n_pairs
    return [min(per, n_pairs - p0) for p0 in range(0, n_pairs, per)]


def word_of(key, L, k):
    """The word whose k-mer key is `key`: its digits in base L, most significant first."""
    assert 0 <= key < L ** k
    out = np.zeros(k, np.uint8)
    for t in range(k - 1, -1, -1):
        key, out[t] = divmod(key, L)
    return out


def key_of(word, L):
    v = 0
    for c in np.asarray(word).tolist():
        v = v * L + int(c)
    return v


def mask_sets(L):
    """Mask sets for the pairwise index: the all-zero word is dropped, and every word of zeros and top letters; with 36
    letters also a set that holds letter 35 alone (bit 35 of the letter set)."""
    return [{0}, {0, L - 1}] + ([{35}] if L == 36 else [])


def _rand(rng, L, n):
    return rng.integers(0, L, n).astype(np.uint8)


def _mutate(rng, x, L, rate):
    """Substitutions at `rate` and indels at `rate` (half deletions, half insertions)."""
    u, sub = rng.random(len(x)), rng.random(len(x)) < rate
    new, ins = rng.integers(0, L, len(x)), rng.integers(0, L, len(x))
    out = []
    for q, c in enumerate(x.tolist()):
        if u[q] < rate / 2:
            continue
        if u[q] < rate:
            out.append(int(ins[q]))
        out.append(int(new[q]) if sub[q] else c)
    return np.array(out, np.uint8)


def _other_letter(rng, c, L):
    return (int(c) + 1 + int(rng.integers(0, L - 1))) % L


def planted_words(rng, L, k):
    """The words a wide input carries: `top` (every letter L - 1: the key L^k - 1), `zero` (key 0), `twice` (put twice into
    either read: four seeds, and an (i, j) order inside one k-mer), the decoys `W` (in S) with `W_first` and `W_last` (in T: W
    with its first, its last letter changed), and, where L^k > 2^33, `a` (in S) and `b` (in T) whose keys differ by exactly
    2^32."""
    w = dict(top=np.full(k, L - 1, np.uint8), zero=np.zeros(k, np.uint8), twice=_rand(rng, L, k), W=_rand(rng, L, k))
    w['W_first'], w['W_last'] = w['W'].copy(), w['W'].copy()
    w['W_first'][0] = _other_letter(rng, w['W'][0], L)
    w['W_last'][-1] = _other_letter(rng, w['W'][-1], L)
    if L ** k > 2 ** 33:
        a = int(rng.integers(0, L ** k - 2 ** 32))
        w['a'], w['b'] = word_of(a, L, k), word_of(a + 2 ** 32, L, k)
    return w


def _join(rng, L, words):
    """The words in a row, three random letters before, between and after them."""
    out = [_rand(rng, L, 3)]
    for w in words:
        out += [w, _rand(rng, L, 3)]
    return np.concatenate(out)


def _sides(rng, w, matching=True):
    """The words of the S side and of the T side.  A decoy of T shares all but a letter or two with its word of S, so the
    letters next to it would make seeds of their own: every decoy carries a letter before and behind it, and those of the T
    side differ from those of the S side."""
    s, t = ([w['top'], w['zero'], w['twice'], w['twice']],) * 2 if matching else ([], [])
    L = int(w['top'][0]) + 1

    def flanked(sw, tws):
        x, y = _rand(rng, L, 2)
        return ([np.concatenate([[x], sw, [y]]).astype(np.uint8)],
                [np.concatenate([[_other_letter(rng, x, L)], tw, [_other_letter(rng, y, L)]]).astype(np.uint8) for tw in tws])
    for sw, tws in ((w['W'], [w['W_first'], w['W_last']]),) + (((w['a'], [w['b']]),) if 'a' in w else ()):
        fs, ft = flanked(sw, tws)
        s, t = s + fs, t + ft
    return s, t


def basic(L, k, seed=0):
    """T: a random stretch of 500 letters, then the planted words; S: the planted words, then a copy of a stretch that
    overlaps T's in 350 letters, mutated at 0.4 %."""
    rng = np.random.default_rng([L, k, 1, seed])
    w = planted_words(rng, L, k)
    G = _rand(rng, L, 650)
    ws, wt = _sides(rng, w)
    S = np.concatenate([_join(rng, L, ws), _mutate(rng, G[150:], L, .004)])
    T = np.concatenate([G[:500], _join(rng, L, wt)])
    return Input('basic' + ('_%d' % seed if seed else ''), 'basic', S, T, L, k, w)


def sparse(L, k, seed=0):
    """Unrelated reads that share the planted words alone."""
    rng = np.random.default_rng([L, k, 2, seed])
    w = planted_words(rng, L, k)
    ws, wt = _sides(rng, w)
    S = np.concatenate([_join(rng, L, ws), _rand(rng, L, 100)])
    T = np.concatenate([_rand(rng, L, 120), _join(rng, L, wt)])
    return Input('sparse' + ('_%d' % seed if seed else ''), 'sparse', S, T, L, k, w)


def empty(L, k):
    """The decoys only: no seed."""
    rng = np.random.default_rng([L, k, 3])
    w = planted_words(rng, L, k)
    ws, wt = _sides(rng, w, matching=False)
    return Input('empty', 'empty', np.concatenate([_rand(rng, L, 60), _join(rng, L, ws)]),
                 np.concatenate([_rand(rng, L, 70), _join(rng, L, wt)]), L, k, w)


def periodic(L, k):
    """0 1 .. p-1 repeated, p = min(L, 7), against the same with another length, the top and zero words behind both: a k-mer
    of S meets every p-th k-mer of T.  The lengths give about 3500 seeds: more than the 2048 a workgroup scores from the seed
    list, fewer than the 5000 the KD-tree oracle of the end-to-end tests holds."""
    rng = np.random.default_rng([L, k, 4])
    w = planted_words(rng, L, k)
    p = min(L, 7)
    a = int(np.ceil(np.sqrt(3200 * p)))
    b = a + a // 10
    tail = [w['top'], w['zero']]
    S = np.concatenate([np.resize(np.arange(p, dtype=np.uint8), a + k - 1), _join(rng, L, tail)])
    T = np.concatenate([np.resize(np.arange(p, dtype=np.uint8), b + k - 1), _join(rng, L, tail)])
    return Input('periodic', 'periodic', S, T, L, k, w)


def doubled(L, k, seed=0):
    """U against U + U, |U| = 200 with the top and zero words inside: the diagonals 0 and -200 hold the same seeds over the
    same expected length."""
    rng = np.random.default_rng([L, k, 5, seed])
    w = planted_words(rng, L, k)
    mid = _join(rng, L, [w['top'], w['zero']])
    U = np.concatenate([_rand(rng, L, 60), mid, _rand(rng, L, 200 - 60 - len(mid))])
    return Input('two_equal_best', 'doubled', U, np.concatenate([U, U]), L, k, w)


@functools.lru_cache(maxsize=None)
def inputs(L, k):
    """The inputs of a rung, by name: basic, sparse, empty, periodic, two_equal_best -- and a second basic and sparse pair
    where a group of five would not fill three chunks of a pair-list call."""
    out = [basic(L, k), sparse(L, k), empty(L, k), periodic(L, k), doubled(L, k)]
    per = pairs_per_chunk(L, k)
    if per is not None and 1 < per < len(out) and len(chunk_sizes(len(out), L, k)) < 3:
        out += [basic(L, k, 1), sparse(L, k, 1)]
    return collections.OrderedDict((x.name, x) for x in out)


# ---- what the CPU test asserts, from the oracle's keys ---------------------------------------------------------------
def keys(x):
    return RO.kmer_keys(x.S, x.wordlen, x.alphabet_len), RO.kmer_keys(x.T, x.wordlen, x.alphabet_len)


def count_seeds(kS, kT):
    """Seeds of a join on these keys: the sum over the keys of S of their hits in T."""
    kT = np.sort(kT)
    return int((np.searchsorted(kT, kS, 'right') - np.searchsorted(kT, kS, 'left')).sum())


def seeds_modulo_2_32(x):
    """The seeds a join would count that compared the low 32 bits of the keys only."""
    kS, kT = keys(x)
    return count_seeds(kS & 0xffffffff, kT & 0xffffffff)


def max_key_bits(x):
    kS, kT = keys(x)
    return int(max(kS.max(), kT.max())).bit_length()


def hits_both_sides(x):
    """The most hits min(on S, on T) of one k-mer."""
    kS, kT = keys(x)
    uS, cS = np.unique(kS, return_counts=True)
    uT, cT = np.unique(kT, return_counts=True)
    _, iS, iT = np.intersect1d(uS, uT, return_indices=True)
    return int(np.minimum(cS[iS], cT[iT]).max()) if len(iS) else 0


def check_input(x):
    """Asserts that the input can tell a wrong join from a right one at its key width."""
    L, k, w = x.alphabet_len, x.wordlen, x.planted
    kS, kT = (set(v.tolist()) for v in keys(x))
    n = count_seeds(*keys(x))
    if x.kind == 'empty':
        assert n == 0
    else:
        assert n > 0 and max_key_bits(x) == key_bits(L, k) == KEY_BITS[(L, k)], x.name
        assert 0 in kS and 0 in kT and L ** k - 1 in kS and L ** k - 1 in kT, x.name
    if x.kind in ('basic', 'sparse', 'periodic'):
        assert hits_both_sides(x) >= 2, x.name
    if x.kind in ('basic', 'sparse', 'empty'):
        # the decoys: one end letter differs, or the keys are equal modulo 2^32 -- no seed
        assert key_of(w['W'], L) in kS and key_of(w['W'], L) not in kT
        assert {key_of(w['W_first'], L), key_of(w['W_last'], L)} <= kT and not {key_of(w['W_first'], L), key_of(w['W_last'], L)} & kS
        assert (w['W_first'][1:] == w['W'][1:]).all() and (w['W_last'][:-1] == w['W'][:-1]).all()
        assert ('a' in w) == (L ** k > 2 ** 33)
        if 'a' in w:
            a, b = key_of(w['a'], L), key_of(w['b'], L)
            assert b - a == 2 ** 32 and a in kS and a not in kT and b in kT and b not in kS
            assert seeds_modulo_2_32(x) != n, x.name
    assert key_type(L, k) == KEY_TYPE[(L, k)]


# ---- the inputs of tests/test_gpu_wide_words.py that are no read pairs ------------------------------------------------
def table_edge_small(n_kmers, seed=0):
    """L = 4, k = 8 around the direct-address table's density bound 4^8 // n <= 64: T (and, for the self comparison, S2) with
    n_kmers k-mers, S a mutated piece of T with a repeat."""
    rng = np.random.default_rng([4, 8, n_kmers, seed])
    T = _rand(rng, 4, n_kmers + 7)
    piece = _mutate(rng, T[300:600], 4, .02)
    S = np.concatenate([piece, np.zeros(10, np.uint8), np.full(10, 3, np.uint8), piece[:40], _rand(rng, 4, 50)])
    T[-20:-10], T[-10:] = 0, 3
    return S, T


def table_edge_large(n_kmers):
    """L = 4, k = 13 around the bound 4^13 // n <= 64 of the largest table (2^26 keys): T with n_kmers k-mers; S of about
    14 kb holds a mutated 6 kb piece of T and the top and zero words, which T ends with."""
    rng = np.random.default_rng([4, 13, 7])
    T = _rand(rng, 4, n_kmers + 12)
    T[-26:-13], T[-13:] = 3, 0
    S = np.concatenate([_rand(rng, 4, 4000), _mutate(rng, T[500000:506000], 4, .004), np.full(13, 3, np.uint8), _rand(rng, 4, 5),
                        np.zeros(13, np.uint8), _rand(rng, 4, 4000)])
    return S, T


def nway(L, k, N, seed=0):
    """N slightly mutated copies of a 300-letter core at different offsets, the top word behind each."""
    rng = np.random.default_rng([L, k, N, seed])
    core = _rand(rng, L, 300)
    return [np.concatenate([_rand(rng, L, int(rng.integers(0, 40))), _mutate(rng, core, L, .003), _rand(rng, L, 3),
                            np.full(k, L - 1, np.uint8), _rand(rng, L, int(rng.integers(0, 20)))]) for _ in range(N)]
