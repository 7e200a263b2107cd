"""Named inputs for the query-batched seed index (kernels K10 of pw_qseeds.hip), each from a fixed RNG seed and each built
to land on one grouping constant, lookup path or radius edge of those kernels: a query that starts on a chosen position
or row, a run of one k-mer across whole 2048-row chunks, queries of exactly 63 / 64 / 65 rows, sort keys whose field
widths change, pairs on and one step past the radius.  tests/test_qseeds_cases.py proves from the dense oracle
(oracle/qseeds_dense_oracle.py) and arithmetic alone that every case lands where it is meant to;
tests/test_gpu_qseeds_edges.py runs the same inputs on the device.

A case is a dict: ``ref`` and ``queries`` (uint8 arrays of letter indices), ``wordlen``, ``L`` (alphabet length) and what
the case is about (``c``, ``R``, ...).  The oracle's rows of a case are cached by its name, computed once and read-only.

Planted inputs (the expand and count cases) are over ACGT at k = 4: the reference is a run of As, a run of Cs and one
GGGG, and holds no T; a query is a string of the words AAAA / CCCC / GGGG with a T between them.  Every k-mer that
touches a T has no hit, so a query's rows are the planted words' runs in the reference -- which is what lets a run, or a
query, be placed on a chosen row.
"""
from functools import lru_cache

import numpy as np

from oracle import qseeds_dense_oracle as QO
from tests import mseeds_cases as MC

MATCH_WG = 256                       # positions per workgroup of k_qmatch (blockIdx.x * 256)
EXP_ROWS = 2048                      # rows per workgroup of k_qexpand (kExpRows)
BOX_WG = 4                           # boxes per workgroup of k_qcount (blockIdx.x * 4: one wavefront each)
BALLOT = 64                          # rows per ballot of k_qcount (base += 64)
TAB_MAX = 1 << 26                    # index_reference: the direct-address table is filled when L^k <= 2^26 ...
TAB_SPARSITY = 64                    # ... and L^k / nk <= 64 (integer division)
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def case(name, ref, queries, wordlen, L, **kw):
    out = dict(name=name, ref=np.asarray(ref, np.uint8), queries=[np.asarray(t, np.uint8) for t in queries], wordlen=wordlen, L=L)
    out.update(kw)
    return out


_ROWS = {}


def rows_of(c):
    """(rows, row offsets) of a case from the dense oracle (cached by the case's name; read-only)."""
    if c['name'] not in _ROWS:
        r, off = QO.rows(c['ref'], c['queries'], c['wordlen'], c['L'])
        r.setflags(write=False)
        off.setflags(write=False)
        _ROWS[c['name']] = (r, off)
    return _ROWS[c['name']]


def lengths(c):
    return np.array([len(t) for t in c['queries']], np.int64)


def pstart(c):
    """First position of every query in (q, j) order, and the position total last: k_qmatch's pstart."""
    return np.concatenate([[0], np.cumsum(lengths(c))]).astype(np.int64)


def pack_tight(queries, slack=16):
    """(arena, offsets, lengths) with the queries back to back, no gap at all between them: the letter behind a query's
    last one is its successor's first."""
    lens = np.array([len(t) for t in queries], np.int32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if len(queries) else np.zeros(0, np.int64)
    arena = np.concatenate([np.asarray(t, np.uint8) for t in queries] + [np.zeros(slack, np.uint8)])
    return arena, offs, lens


def lookup_of(L, k, nref):
    """The join k_qmatch takes, restated from pw_qseeds_create / index_reference: 'table', 'search32' or 'search64'."""
    kinv = L ** k
    nk = nref - k + 1
    if not kinv < 0xffffffff:
        return 'search64'
    return 'table' if kinv <= TAB_MAX and kinv // nk <= TAB_SPARSITY else 'search32'


def bits_for(maxval):
    """pw_hip_host.h's bits_for: the width of a sort-key field that holds 0 .. maxval."""
    b = 1
    while maxval >> b:
        b += 1
    return b


def _mutate(rng, s, rate=.06):
    s = np.array(s, np.uint8)
    flip = rng.random(len(s)) < rate
    s[flip] = (s[flip] + rng.integers(1, 4, int(flip.sum()))) % 4
    return s


# ---- k_qmatch ------------------------------------------------------------------------------------------------
POSITION_EDGES = (255, 256, 257, 511, 512, 513)
MATCH_K = 6


@lru_cache(None)
def query_edge_at_position(p):
    """Query 2 starts on position p.  Query 1 ends with the word ref[200:206] and query 2 goes on with ref[206:...]: in an
    arena packed with no gaps every k-mer across the boundary is a word of the reference."""
    rng = np.random.default_rng(9800 + p)
    k, x = MATCH_K, 200
    ref = rng.integers(0, 4, 500)
    q1 = np.r_[rng.integers(0, 4, p - 90 - k), ref[x:x + k]]
    return case('query_edge_at_position_%d' % p, ref, [rng.integers(0, 4, 90), q1, ref[x + k:x + k + 60], rng.integers(0, 4, 30)],
                k, 4, c=4., R=12., edge_query=2)


@lru_cache(None)
def many_queries_in_one_workgroup():
    """120 queries of 0 .. 3 letters at k = 2 (every third one empty), then one of 700 letters."""
    rng = np.random.default_rng(9810)
    ref = rng.integers(0, 4, 40)
    short = [rng.integers(0, 4, 0 if q % 3 == 1 else int(rng.integers(1, 4))) for q in range(120)]
    return case('many_queries_in_one_workgroup', ref, short + [rng.integers(0, 4, 700)], 2, 4, c=1., R=3.)


@lru_cache(None)
def empties_at_a_window_edge():
    rng = np.random.default_rng(9811)
    ref = rng.integers(0, 4, 400)
    e = np.zeros(0, np.uint8)
    return case('empties_at_a_window_edge', ref, [e, e, e, _mutate(rng, ref[20:20 + MATCH_WG]), e, e, e, e, _mutate(rng, ref[250:350]),
                                                  e, e, e], MATCH_K, 4, c=4., R=12.)


NPOS = (255, 256, 257, 1)


@lru_cache(None)
def npos_around_a_workgroup(n):
    """The queries' lengths sum to n; the last query is a slice of the reference (n = 1: one letter)."""
    rng = np.random.default_rng(9820 + n)
    ref = rng.integers(0, 4, 400)
    e = np.zeros(0, np.uint8)
    queries = [np.array([2])] if n == 1 else [_mutate(rng, ref[10:110]), e, _mutate(rng, ref[120:120 + n - 140]), ref[300:340]]
    return case('npos_around_a_workgroup_%d' % n, ref, queries, MATCH_K, 4, c=4., R=12.)


# name -> (L, k, reference length)
LOOKUPS = {'table': (4, 6, 300), 'table_edge': (4, 6, 64 + 5), 'sparse32': (4, 6, 63 + 5), 'big32': (4, 14, 300),
           'odd32': (3, 20, 300), 'first64': (4, 16, 300), 'wide64': (4, 30, 300), 'letters36': (36, 11, 300)}
LOOKUP_PATH = {'table': 'table', 'table_edge': 'table', 'sparse32': 'search32', 'big32': 'search32', 'odd32': 'search32',
               'first64': 'search64', 'wide64': 'search64', 'letters36': 'search64'}


@lru_cache(None)
def lookup_path(name, present):
    """The queries hold key 0 (k times letter 0) and key L^k - 1 (k times letter L - 1).  ``present``: the reference holds
    both words, once each; otherwise it holds neither, and the two are a k-mer below and one above every key it has."""
    L, k, nref = LOOKUPS[name]
    rng = np.random.default_rng(9830 + sorted(LOOKUPS).index(name) * 2 + int(present))
    body = rng.integers(0, L, nref)
    for i in range(nref):                        # no run of k zeros and none of k times L - 1 in the random part
        if i >= k - 1 and (body[i - k + 1:i + 1] == 0).all() or i >= k - 1 and (body[i - k + 1:i + 1] == L - 1).all():
            body[i] = 1
    if present:
        body[:k + 1] = [0] * k + [1]
        body[-k - 1:] = [L - 2] + [L - 1] * k
    at = min(10, nref - k - 20)
    queries = [body[at:at + k + 20], np.r_[[0] * k, [L - 1] * k], rng.integers(0, L, k + 10), np.zeros(k, np.uint8),
               np.full(k + 1, L - 1)]
    return case('lookup_%s_%d' % (name, present), body, queries, k, L, c=1., R=4., present=present)


# ---- planted inputs ------------------------------------------------------------------------------------------
PLANT_K, PLANT_M = 4, 100            # word length; hits of CCCC in the planted reference


def planted_ref(n_a):
    """AAAA n_a times (a run of n_a + 3 As), CCCC PLANT_M times, GGGG once; no T."""
    return np.r_[[0] * (n_a + 3), [1] * (PLANT_M + 3), [2] * 4].astype(np.uint8)


def words(n):
    """A query of exactly n rows against planted_ref: n // PLANT_M times CCCC, then n % PLANT_M times GGGG, a T before,
    between and behind them."""
    out = [3]
    for _ in range(n // PLANT_M):
        out += [1, 1, 1, 1, 3]
    for _ in range(n % PLANT_M):
        out += [2, 2, 2, 2, 3]
    return np.array(out, np.uint8)


# ---- k_qexpand -----------------------------------------------------------------------------------------------
CHUNK_EDGES = (EXP_ROWS - 1, EXP_ROWS, EXP_ROWS + 1)
RUN = 2 * EXP_ROWS + 104             # hits of AAAA in run_across_chunks' reference


@lru_cache(None)
def run_across_chunks(start):
    """Query 1's AAAA has RUN rows, the first of them row `start`; the positions before and behind it have no hit."""
    queries = [words(1000), np.r_[words(start - 1000), [0, 0, 0, 0], words(7)], words(130)]
    return case('run_across_chunks_%d' % start, planted_ref(RUN), queries, PLANT_K, 4, start=start)


@lru_cache(None)
def query_edge_at_row(r):
    e = np.zeros(0, np.uint8)
    return case('query_edge_at_row_%d' % r, planted_ref(10), [words(r), words(150), e, words(3)], PLANT_K, 4, c=1., R=5., edge_query=1)


TOTALS = (2047, 2048, 2049, 1)


@lru_cache(None)
def total_rows(n):
    e = np.zeros(0, np.uint8)
    queries = [words(0), words(1)] if n == 1 else [words(n - 201), e, words(200), words(1)]
    return case('total_rows_%d' % n, planted_ref(10), queries, PLANT_K, 4, c=1., R=5.)


# ---- k_qcount ------------------------------------------------------------------------------------------------
LADDER = (0, 1, 63, 64, 65, 128, 129)


@lru_cache(None)
def rows_per_query_ladder():
    return case('rows_per_query_ladder', planted_ref(10), [words(n) for n in LADDER], PLANT_K, 4, c=1., R=5.)


BOX_BATCHES = (0, 1, 3, 4, 5, 257)
BOX_ALWAYS_ZERO = ('inverted_d', 'inverted_a', 'empty_query')
_EDGE_W = 3


def boxes(c, n_boxes, seed):
    """n_boxes boxes on the rows of case c: dict of int32 arrays q, dmin, dmax, amin, amax and the list ``kind``; a smaller
    batch is a prefix.  First, around one row (d, a) of the query with the most rows: that row on the box's dmin, dmax,
    amin, amax edge, each followed by the box one step further in, which leaves it outside.  Then bounds inverted on d and
    on a, the whole int32 plane on every query (kind 'empty_query' where the query has no rows), five boxes on one query,
    and random boxes on random queries: the query order is scrambled."""
    rng = np.random.default_rng(seed)
    rows, off = rows_of(c)
    per_q = np.diff(off)
    nq = len(per_q)
    out = []
    big = int(np.argmax(per_q))
    r = rows[off[big] + per_q[big] // 2]
    d, a, w = int(r[1]), int(r[2]), _EDGE_W
    for name, box in (('dmin', (d, d + w, a - w, a + w)), ('dmax', (d - w, d, a - w, a + w)), ('amin', (d - w, d + w, a, a + w)),
                      ('amax', (d - w, d + w, a - w, a))):
        out.append((name + '_edge', big) + box)
        step = {'dmin': (1, 0, 0, 0), 'dmax': (0, -1, 0, 0), 'amin': (0, 0, 1, 0), 'amax': (0, 0, 0, -1)}[name]
        out.append((name + '_out', big) + tuple(x + s for x, s in zip(box, step)))
    out.append(('inverted_d', big, d + 1, d, I32_MIN, I32_MAX))
    out.append(('inverted_a', big, I32_MIN, I32_MAX, a + 1, a))
    for q in rng.permutation(nq).tolist():
        out.append(('plane' if per_q[q] else 'empty_query', q, I32_MIN, I32_MAX, I32_MIN, I32_MAX))
    have = np.flatnonzero(per_q)
    while len(out) < n_boxes:
        several = len([x for x in out if x[0] == 'several']) < 5
        q = big if several else int(rng.integers(0, nq))
        if per_q[q] == 0:
            q = int(have[rng.integers(0, len(have))]) if rng.random() < .7 else q
        pr = rows[rng.integers(off[q], off[q + 1])] if per_q[q] else (q, 0, 0)
        out.append(('several' if several else 'random', q, int(pr[1]) - int(rng.integers(0, 30)), int(pr[1]) + int(rng.integers(0, 30)),
                    int(pr[2]) - int(rng.integers(0, 200)), int(pr[2]) + int(rng.integers(0, 200))))
    out = out[:n_boxes]
    cols = list(zip(*out)) if out else [[]] * 6
    res = {f: np.array(cols[i + 1], np.int64).astype(np.int32) for i, f in enumerate(('q', 'dmin', 'dmax', 'amin', 'amax'))}
    res['kind'] = list(cols[0])
    return res


def box_counts(c, b):
    rows, off = rows_of(c)
    return QO.box_counts(rows, off, b['q'], b['dmin'], b['dmax'], b['amin'], b['amax'])


# ---- k_qgraph_* ----------------------------------------------------------------------------------------------
GRAPH_K = 6


def _fill(rng, n):
    """n letters over G and T: no run of As or Cs goes on into it."""
    return rng.integers(2, 4, n)


def _cornered_ref(rng, nR):
    """k + 1 As, random letters (the first no A, the last no C), k + 1 Cs: AAAAAA stands at 0 and 1, CCCCCC at nR - k - 1
    and nR - k."""
    k = GRAPH_K
    mid = rng.integers(0, 4, nR - 2 * (k + 1))
    mid[0], mid[-1] = 2, 3
    return np.r_[[0] * (k + 1), mid, [1] * (k + 1)]


@lru_cache(None)
def corners():
    """Query 1 (150 letters, the longest; the reference has 61) starts with the Cs the reference ends with and ends with the
    As it starts with; query 2, as long, ends with the Cs."""
    rng = np.random.default_rng(9840)
    k, nR, n = GRAPH_K, 61, 150
    ref = _cornered_ref(rng, nR)
    q1 = np.r_[[1] * (k + 1), _fill(rng, n - 2 * (k + 1)), [0] * (k + 1)]
    q2 = np.r_[_fill(rng, n - (k + 1)), [1] * (k + 1)]
    return case('corners', ref, [np.zeros(0, np.uint8), q1, q2, ref[10:40]], k, 4, c=1., R=2.)


FIELD_SUMS, FIELD_NQ = (255, 256, 257), (1, 2, 3, 257)
FIELD_NR = 155


@lru_cache(None)
def field_widths(s, nq):
    """nR + the longest query's length = s, nq queries.  The last query is the longest and holds both extreme diagonals
    (as corners' query 1); the others are mutated slices of the reference."""
    rng = np.random.default_rng(9850 + 4 * s + FIELD_NQ.index(nq))
    k, nR = GRAPH_K, FIELD_NR
    ref = _cornered_ref(rng, nR)
    n = s - nR
    inner = n - 2 * (k + 1)
    at = int(rng.integers(k + 1, nR - k - 1 - inner))
    last = np.r_[[1] * (k + 1), [2], _mutate(rng, ref[at:at + inner - 2], .04), [3], [0] * (k + 1)]
    queries = []
    for _ in range(nq - 1):
        ln = int(rng.integers(20, 61))
        at = int(rng.integers(0, nR - ln))
        queries.append(_mutate(rng, ref[at:at + ln], .04))
    return case('field_widths_%d_%d' % (s, nq), ref, queries + [last], k, 4, c=1., R=6., s=s)


@lru_cache(None)
def twins():
    """Queries 1 and 2 are the same letters."""
    rng = np.random.default_rng(9860)
    ref = rng.integers(0, 4, 300)
    t = _mutate(rng, ref[50:250], .05)
    return case('twins', ref, [_mutate(rng, ref[10:90]), t, t.copy(), _mutate(rng, ref[200:290])], GRAPH_K, 4, c=4., R=12.)


NEAR_D, NEAR_A = MC.NEAR_D, MC.NEAR_A              # d_radius, a_radius: c = 30 / 7 is inexact in binary
NEAR_L, NEAR_K = 36, 5


def _word(j):
    return [(j >> (2 * (NEAR_K - 1 - t))) & 3 for t in range(NEAR_K)]


@lru_cache(None)
def near_miss_d(delta):
    """Word 1 stands at 60 and 60 + delta in the reference and once in query 1: its two seeds differ by delta in d and in
    a.  delta = NEAR_D is on the radius, NEAR_D + 1 one step past it.  The query's lead-in is chosen so that fl(d c) lands
    on the side of R the exact product is on (the rounding cases are for the other diagonals).  Word 2, 400 letters on,
    stands once in query 0."""
    rng = np.random.default_rng(9870 + delta)
    c = 1. * NEAR_A / NEAR_D
    i0 = 60
    j0 = next(j for j in range(int(rng.integers(1, 20)), i0)
              if MC.lands(i0 + NEAR_D - j, NEAR_D, c, NEAR_A) and not MC.lands(i0 + NEAR_D + 1 - j, NEAR_D + 1, c, NEAR_A))
    sp_r = lambda n: rng.integers(4, 6, n).tolist()           # noqa: E731
    sp_q = lambda n: rng.integers(6, 8, n).tolist()           # noqa: E731
    ref = sp_r(i0) + _word(1) + sp_r(delta - NEAR_K) + _word(1) + sp_r(400) + _word(2) + sp_r(3)
    queries = [sp_q(5) + _word(2) + sp_q(2), sp_q(j0) + _word(1) + sp_q(4)]
    return case('near_miss_d_%d' % delta, ref, queries, NEAR_K, NEAR_L, c=c, R=float(NEAR_A), delta=delta)


NEAR_T = 9


@lru_cache(None)
def near_miss_a():
    """Word 1 twice, NEAR_T letters apart, in the reference and in query 1: four seeds, of which (i, j) and (i + t, j + t)
    share d and differ by 2 t in a.  With c = 2 t every other pair is t * 2 t apart on the d axis."""
    rng = np.random.default_rng(9880)
    sp_r = lambda n: rng.integers(4, 6, n).tolist()           # noqa: E731
    sp_q = lambda n: rng.integers(6, 8, n).tolist()           # noqa: E731
    t = NEAR_T
    ref = sp_r(33) + _word(1) + sp_r(t - NEAR_K) + _word(1) + sp_r(200) + _word(2) + sp_r(3)
    queries = [sp_q(5) + _word(2) + sp_q(2), sp_q(12) + _word(1) + sp_q(t - NEAR_K) + _word(1) + sp_q(4)]
    return case('near_miss_a', ref, queries, NEAR_K, NEAR_L, c=2. * t, R=2. * t, R_past=2. * t - 1)


def _runs(rng, name, d0, **kw):
    """AAAAAA at i0, i0 + 1, i0 + 2 in the reference and at j0, j0 + 1 in query 1, i0 - j0 = d0: six seeds, among them
    (i0, j0 + 1) and (i0 + 2, j0) -- diagonals d0 - 1 and d0 + 2, a one apart -- and (i0, j0), (i0 + 1, j0 + 1), (i0 + 2, j0 + 1)
    -- a two and three apart."""
    k, i0 = GRAPH_K, 40
    j0 = i0 - d0
    ref = np.r_[rng.integers(1, 3, i0), [0] * (k + 2), rng.integers(1, 3, 20)]       # Cs and Gs around the run; Ts in the queries
    queries = [np.r_[[3] * 9, [0] * k, [3] * 3], np.r_[[3] * j0, [0] * (k + 1), [3] * 15]]
    return case(name, ref, queries, k, 4, d0=d0, **kw)


@lru_cache(None)
def non_integer_radius():
    return _runs(np.random.default_rng(9890), 'non_integer_radius', 11, c=1., R=2.5)


# A pair of seeds of two sequences has d and a of the same parity: the pairs three diagonals apart are one apart in a,
# never zero, and R = MC.ROUND_R < 1 would cut them on the a axis.  Scaling c and R by 4 is exact in binary --
# fl(d 4c) = 4 fl(d c) -- so the d axis decides exactly as with MC's constants, and |a - a'| = 1 <= 4 R passes.
ROUND_SCALE = 4
ROUNDINGS = ((MC.ROUND_C, MC.ROUND_R, MC.ROUNDING_D0[0]), (MC.ROUND_C, MC.ROUND_R, MC.ROUNDING_D0[1]), MC.ROUNDING_OTHER_WAY)


@lru_cache(None)
def rounding(which):
    c0, R0, d0 = ROUNDINGS[which]
    return _runs(np.random.default_rng(9900 + which), 'rounding_%d' % which, d0, c=ROUND_SCALE * c0, R=ROUND_SCALE * R0, c0=c0, R0=R0)


@lru_cache(None)
def radius_zero():
    c = dict(field_widths(256, 3))
    c.update(name='radius_zero', c=1., R=0.)
    return c


@lru_cache(None)
def window_clamped():
    """floor(R / c) + 2 = 10^6 + 2 diagonals either way, and the table has 71."""
    rng = np.random.default_rng(9910)
    return case('window_clamped', rng.integers(0, 4, 40), [rng.integers(0, 4, 30), rng.integers(0, 4, 25)], 3, 4, c=1e-3, R=1000.)


CHAIN_M, CHAIN_K, CHAIN_STRIDE = 40, 12, 1000
CHAIN_R = float(CHAIN_STRIDE + CHAIN_M * CHAIN_K)


@lru_cache(None)
def chain():
    """CHAIN_M random 12-mers stand CHAIN_STRIDE letters apart in the reference; each of the two queries is those words
    back to back in an order of its own (a word starts and ends with A, the letters around it in the reference are Ts: no
    shifted k-mer matches).  Row p of a query (its p-th word, word w) has a = CHAIN_STRIDE w + 12 p: at
    R = CHAIN_STRIDE + 12 CHAIN_M a row is connected to the rows of words w - 1 and w + 1 and to nothing else, so each
    query is one path whose rows come scrambled along it."""
    rng = np.random.default_rng(9923)
    blocks = [np.r_[0, rng.integers(0, 4, CHAIN_K - 2), 0] for _ in range(CHAIN_M)]       # A first and last, and the filler
    ref = np.concatenate([np.r_[b, 3, rng.integers(0, 4, CHAIN_STRIDE - CHAIN_K - 2), 3] for b in blocks])   # T first and last
    perms = [rng.permutation(CHAIN_M) for _ in range(2)]
    queries = [np.concatenate([blocks[w] for w in p]) for p in perms]
    return case('chain', ref, queries, CHAIN_K, 4, c=1., R=CHAIN_R, perms=perms)


def chain_masks(n):
    return MC.chain_masks(n)
