"""Named stranded inputs for the query-batched seed index (k_qmatch_stranded of pw_qseeds.hip, pw_qseeds_build_stranded).

A stranded case is a case of tests/qseeds_cases.py -- ``ref``, ``wordlen``, ``L``, ``c``, ``R`` and ``queries`` -- whose
``queries`` are the listed entries AS THE INDEX MUST SEE THEM: the reverse complement, materialised here on the host, where
the entry's strand is minus.  So ``qseeds_cases.rows_of`` (the dense oracle, which knows nothing of strands) gives the rows
the device must produce.  What the device is handed instead: ``base`` (forward letters, uint8 arrays), ``source`` (entry ->
index into ``base``: two entries may name the same letters), ``strands`` (one 0 / 1 per entry) and ``comp`` (the
complement table).  tests/test_qseeds_strand_cases.py proves on the CPU that each case does what it is for;
tests/test_gpu_qseeds_strands.py runs them on the device.
"""
from functools import lru_cache
from itertools import product

import numpy as np

from tests import qseeds_cases as QC

COMP4 = (3, 2, 1, 0)                                  # ACGT: A <-> T, C <-> G
PATTERNS = ('minus', 'alternating', 'twice')


def rc(t, comp):
    return np.asarray(comp, np.uint8)[np.asarray(t, np.int64)[::-1]]


def stranded(name, ref, base, source, strands, wordlen, L, comp, **kw):
    base = [np.asarray(t, np.uint8) for t in base]
    seen = [rc(base[s], comp) if f else base[s] for s, f in zip(source, strands)]
    return QC.case(name, ref, seen, wordlen, L, base=base, source=list(source), strands=np.asarray(strands, np.uint8),
                   comp=np.asarray(comp, np.uint8), **kw)


def listing(sc, pack=QC.pack_tight):
    """(arena, offsets, lengths) of the listed entries over ONE copy of the base letters."""
    arena, offs, lens = pack(sc['base'])
    return arena, np.asarray(offs, np.int64)[sc['source']], np.asarray(lens, np.int32)[sc['source']]


def with_strands(c, pattern, comp=COMP4):
    """A case of qseeds_cases under a strand pattern.  'minus' (every entry) and 'alternating' (+, -, +, ...): a minus entry
    is handed the reverse complement of the case's query, so what the index must see -- and every row -- is the case's own.
    'twice': every query listed on both strands, + then -, over the same letters."""
    n = len(c['queries'])
    extra = {f: c[f] for f in ('c', 'R') if f in c}
    if pattern == 'twice':
        return stranded('%s_twice' % c['name'], c['ref'], c['queries'], [q for q in range(n) for _ in (0, 1)], [0, 1] * n,
                        c['wordlen'], c['L'], comp, **extra)
    flags = [1] * n if pattern == 'minus' else [q % 2 for q in range(n)]
    base = [rc(t, comp) if f else t for t, f in zip(c['queries'], flags)]
    return stranded('%s_%s' % (c['name'], pattern), c['ref'], base, range(n), flags, c['wordlen'], c['L'], comp, **extra)


# ---- lengths around k ----------------------------------------------------------------------------------------
@lru_cache(None)
def lengths_around_k():
    """k = 3 over a 40-letter reference; per length 0 .. 6 a slice of the reference and the reverse complement of another,
    each listed on both strands: 28 entries, 84 positions, one workgroup."""
    rng = np.random.default_rng(9930)
    ref = rng.integers(0, 4, 40)
    base = []
    for n in range(7):
        base += [ref[3 * n:3 * n + n], rc(ref[20 + 2 * n:20 + 2 * n + n], COMP4)]
    return stranded('lengths_around_k', ref, base, [q for q in range(14) for _ in (0, 1)], [0, 1] * 14, 3, 4, COMP4, c=1., R=3.)


# ---- boundary traps ------------------------------------------------------------------------------------------
TRAP_K = 4


def trap_words(A, B, C, k=TRAP_K, comp=COMP4):
    """The k-mers an off-by-one on the minus strand would form across A|B and B|C (the three lie back to back), by the entry
    and the direction of the slip: a frame one letter too far left ends, reversed, on its left neighbour's last letter;
    one too far right starts, reversed, with its right neighbour's first."""
    return {('B', 'left'): rc(np.r_[A[-1:], B[:k - 1]], comp), ('B', 'right'): rc(np.r_[B[-(k - 1):], C[:1]], comp),
            ('A', 'right'): rc(np.r_[A[-(k - 1):], B[:1]], comp), ('C', 'left'): rc(np.r_[B[-1:], C[:k - 1]], comp)}


@lru_cache(None)
def _trap_letters():
    rng = np.random.default_rng(9931)
    A, B, C = (rng.integers(0, 4, n) for n in (11, 9, 10))
    words = trap_words(A, B, C)
    forward = [np.r_[A[-(TRAP_K - 1):], B[:1]], np.r_[B[-(TRAP_K - 1):], C[:1]]]        # the plus strand's slips (as K10a's)
    ref = np.concatenate([rng.integers(0, 4, 20)] + [words[w] for w in sorted(words)] + forward +
                         [A[3:9], rc(A, COMP4)[2:8], B[1:7], rc(B, COMP4)[2:8], C[2:8], rc(C, COMP4)[1:7]])      # rows on either strand
    return ref, (A, B, C)


@lru_cache(None)
def boundary_traps(assign):
    """A | B | C with no gap, strands ``assign`` (three 0 / 1); the reference holds every word of trap_words."""
    ref, base = _trap_letters()
    return stranded('boundary_traps_%d%d%d' % assign, ref, base, range(3), assign, TRAP_K, 4, COMP4, c=1., R=4.)


ASSIGNMENTS = tuple(product((0, 1), repeat=3))


def slipped(sc, entry, by):
    """The rows the oracle gives when minus entry ``entry`` is read from a frame ``by`` letters off (-1: left, 1: right)."""
    arena, offs, lens = listing(sc)
    seen = list(sc['queries'])
    assert sc['strands'][entry] == 1
    seen[entry] = rc(arena[offs[entry] + by:offs[entry] + by + lens[entry]], sc['comp'])
    return QC.QO.rows(sc['ref'], seen, sc['wordlen'], sc['L'])


# ---- alphabets -----------------------------------------------------------------------------------------------
ALPHABETS = {2: (1, 0), 3: (2, 1, 0), 5: (3, 2, 1, 0, 4)}           # the swap; one fixed point; ACGT + N
ALPHABET_K = {2: 7, 3: 5, 5: 4}


@lru_cache(None)
def alphabet_case(L):
    rng = np.random.default_rng(9940 + L)
    k, comp = ALPHABET_K[L], ALPHABETS[L]
    ref = rng.integers(0, L, 300)
    seen = [ref[20:90], rng.integers(0, L, 50), ref[100:100 + k], ref[150:230], np.zeros(0, np.uint8), ref[240:300]]
    c = QC.case('alphabet_%d' % L, ref, seen, k, L, c=2., R=8.)
    return with_strands(c, 'alternating', comp)


@lru_cache(None)
def palindromes():
    """Every k-mer (k = 2) of every query is its own reverse complement, and so is every query: the minus entry of a query
    has the rows of its plus entry."""
    ref = np.array([0, 3] * 10 + [1, 2] * 5 + [0, 0, 1, 1], np.uint8)
    base = [np.array([0, 3] * 3), np.array([1, 2] * 2), np.array([3, 0] * 2), np.array([2, 1] * 3)]
    return stranded('palindromes', ref, base, [q for q in range(4) for _ in (0, 1)], [0, 1] * 4, 2, 4, COMP4, c=1., R=3.)


# ---- lookup paths --------------------------------------------------------------------------------------------
STRAND_LOOKUPS = ('table', 'big32', 'first64', 'letters36')           # table, search32, search64 (k = 16 over 4), search64


def lookup_case(name, pattern):
    c = QC.lookup_path(name, True)
    return with_strands(c, pattern, tuple(range(c['L'] - 1, -1, -1)))


# ---- the mixed sets of blot_many_cases, every odd-numbered query reverse-complemented ------------------------
@lru_cache(None)
def flipped_mixed(name, n=30):
    """(ref, queries, wordlen, K_min, p_min) of ``blot_many_cases.mixed_case(name, n)`` with queries 1, 3, 5, ... replaced by
    their reverse complements: reads from both strands of the molecule."""
    from tests import blot_many_cases as Cs
    ref, queries, wordlen, K_min, p_min = Cs.mixed_case(name, n)
    return ref, [rc(t, COMP4) if q % 2 else t for q, t in enumerate(queries)], wordlen, K_min, p_min


@lru_cache(None)
def flipped_expected(name, n=30):
    """Per query of flipped_mixed the CPU oracle's segments of (the query as given, its reverse complement); computed once
    and shared, read-only."""
    from tests import blot_many_cases as Cs
    ref, queries, wordlen, K_min, p_min = flipped_mixed(name, n)
    return [(Cs.oracle_segments(ref, t, wordlen, K_min, p_min), Cs.oracle_segments(ref, rc(t, COMP4), wordlen, K_min, p_min))
            for t in queries]


def strand_census(name, n=30):
    """(queries with segments on + only, on - only, on both) of flipped_mixed, from the CPU oracle."""
    exp = flipped_expected(name, n)
    return (sum(bool(p) and not m for p, m in exp), sum(bool(m) and not p for p, m in exp), sum(bool(p) and bool(m) for p, m in exp))
