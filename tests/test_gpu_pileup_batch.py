"""The pileups of a batch (``BatchAligner.pileup_add``, ``Pileup``; include/pw_pileup.h) against the oracle of
tests/pileup_ref.py applied to ``b.transcripts(res)`` and ``res`` of the same batch: every comparison is ``==`` on integer
counts.  Colliding wavefronts for every alignment type, the edges of the kernel's dword scan, ``col0``, a smaller alphabet,
the strip pipeline, a traceback from other end cells, the refusals, and ``call`` against the numpy oracle."""
import numpy as np
import pytest

from tests import pileup_ref as R
from tests.helpers import dec, kw_of, load_golden

pytestmark = pytest.mark.gpu

SCORES = dict(match_score=1, mismatch_score=-3, go_score=-5, ge_score=-2)
# gaps cheaper than a substitution: a replaced letter aligns as an insertion directly followed by a deletion
GAPPY = dict(match_score=1, mismatch_score=-20, go_score=-2, ge_score=-1)


def _geometry(b):
    """(origin_off, mutant_off, X, Y) of every pair of a batch, from the pair records it was created with."""
    p = b._pairs
    if isinstance(p, np.ndarray):
        return [(int(r['origin_off']), int(r['mutant_off']), int(r['origin_len']), int(r['mutant_len'])) for r in p[:b.n]]
    return [(int(p[k].origin_off), int(p[k].mutant_off), int(p[k].origin_len), int(p[k].mutant_len)) for k in range(b.n)]


def _expected(b, res, txs, n_cols, L, col0=None, arena_first=0):
    """The oracle's pileup of a batch whose letters are all in its host arena."""
    geo = _geometry(b)
    frames = [g[0] - arena_first for g in geo] if col0 is None else list(col0)
    mutants = [b.arena[g[1]:g[1] + g[3]] for g in geo]
    return R.of_batch(n_cols, L, res, txs, frames, mutants, [g[2] for g in geo])


@pytest.fixture(scope='module')
def reads():
    """One 300-letter origin over two letters and 64 windows of it: mutated copies, and every eighth one shifted to the other
    two letters -- no letter in common with the origin.  Every second window is nearly the whole origin, so that the band
    (-25, 25) of the banded types holds its corners.  ``(arena, offs, lens, pairs)`` for ``from_arena``."""
    from biseqt_amd import synth
    from biseqt_amd.batch import pack_reads
    rng = synth.rng_for(7301)
    origin = (synth.rand_seqs(rng, 1, 300)[0] % 2).astype(np.uint8)
    rs = [origin]
    for k in range(64):
        n = int(rng.integers(285, 301)) if k % 2 == 0 else int(rng.integers(30, 201))
        s = int(rng.integers(0, 300 - n + 1))
        w = origin[s:s + n]
        rs.append(((w + 2) % 4).astype(np.uint8) if k % 8 == 7 else synth.mutate(rng, w, 0.08, 0.04, 0.4))
    arena, offs, lens = pack_reads(rs)
    return arena, offs, lens, np.array([(0, 1 + k) for k in range(64)], np.int64)


def _run_type(reads, mode, alntype):
    """Solve the colliding batch; returns (counts of the device, counts of the oracle, res, txs)."""
    from biseqt_amd.batch import BatchAligner, Pileup
    arena, offs, lens, pairs = reads
    kw = dict(diag_ranges=[(-25, 25)] * len(pairs), check_band=False) if mode == 1 else {}
    with BatchAligner.from_arena(arena, offs, lens, pairs, alnmode=mode, alntype=alntype, alphabet_len=4, **SCORES, **kw) as b, \
            Pileup(300, 4) as p:
        res = b.run()
        txs = b.transcripts(res)
        b.pileup_add(p)
        b.sync()
        return p.counts(), _expected(b, res, txs, 300, 4), res, txs


@pytest.fixture(scope='module')
def global_counts(reads):
    return _run_type(reads, 0, 0)[0]


@pytest.mark.parametrize('alntype', range(7))
def test_colliding_wavefronts_standard_types(reads, alntype):
    from biseqt_amd import _pwlib as W
    got, want, res, txs = _run_type(reads, 0, alntype)
    assert sum(1 for t in txs if t) >= 20
    assert want.max() >= 8                                    # wavefronts do collide on columns
    assert (got == want).all(), np.argwhere(got != want)[:8]
    if alntype == W.LOCAL:                                    # nothing in common under LOCAL: no alignment, no contribution
        for k in range(7, 64, 8):
            assert txs[k] is None and res['tx_len'][k] <= 0, (k, txs[k])
    if alntype == W.GLOBAL:
        assert got[:, 4].any() and got[:, 5].any()            # deletions and insertion events are present


@pytest.mark.parametrize('alntype', range(3))
def test_colliding_wavefronts_banded_types(reads, alntype):
    got, want, res, txs = _run_type(reads, 1, alntype)
    assert sum(1 for t in txs if t) >= 20
    assert (got == want).all(), np.argwhere(got != want)[:8]


SCAN_LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 258, 259, 511, 512, 513)


def scan_edge_pairs():
    """GLOBAL pairs whose transcripts have exactly SCAN_LENGTHS ops, built from a random template by deleting or inserting a
    block at a chosen place (under GAPPY scores the optimal alignment is the construction: all matches and the one gap run,
    so the transcript has max(X, Y) ops) -- or, for 'replace', by replacing one letter (an I directly followed by a D: X + 1
    ops)."""
    from biseqt_amd import synth
    rng = synth.rng_for(7302)

    def other(letter):
        return np.uint8((int(letter) + 2) % 4)

    plan = {1: ('same', 0, 0), 2: ('ins', 0, 1), 3: ('del', 0, 1), 4: ('ins', -1, 1), 5: ('replace', 1, 1),
            63: ('del', 30, 2), 64: ('ins', 61, 3), 65: ('replace', 63, 1), 255: ('ins', -1, 3), 256: ('del', 0, 5),
            257: ('ins', 254, 3), 258: ('del', 255, 2), 259: ('ins', 0, 4), 511: ('ins', 250, 8), 512: ('ins', 251, 8),
            513: ('ins', 252, 6)}
    pairs = []
    for n in SCAN_LENGTHS:
        kind, at, g = plan[n]
        if kind == 'same':
            t = synth.rand_seqs(rng, 1, n)[0]
            pairs.append((t, t.copy()))
            continue
        if kind == 'replace':                                  # X = n - 1 letters, one of them replaced: n ops
            t = synth.rand_seqs(rng, 1, n - 1)[0]
            m = t.copy()
            m[at] = other(t[at])
            pairs.append((t, m))
            continue
        long = synth.rand_seqs(rng, 1, n)[0]                   # the longer sequence; the shorter lacks long[at:at + g]
        at = n - g if at < 0 else at
        # the block must not slide: its first letter differs from the letter behind the block, its last from the one in front
        left = {int(long[at - 1])} if at > 0 else set()
        right = {int(long[at + g])} if at + g < n else set()
        if g == 1:
            long[at] = min(set(range(4)) - left - right)
        else:
            long[at], long[at + g - 1] = min(set(range(4)) - right), min(set(range(4)) - left)
        short = np.concatenate([long[:at], long[at + g:]])
        pairs.append((short, long) if kind == 'ins' else (long, short))
    return pairs


def _gap_runs(tx, op):
    runs, k = [], 0
    while k < len(tx):
        if tx[k] == op:
            s = k
            while k < len(tx) and tx[k] == op:
                k += 1
            runs.append((s, k))
        else:
            k += 1
    return runs


def test_scan_edges():
    from biseqt_amd.batch import BatchAligner, Pileup
    pairs = scan_edge_pairs()
    with BatchAligner(pairs, alnmode=0, alntype=0, alphabet_len=4, **GAPPY) as b, Pileup(b.arena.nbytes, 4) as p:
        res = b.run()
        txs = b.transcripts(res)
        assert [len(t) for t in txs] == list(SCAN_LENGTHS), [len(t or '') for t in txs]
        off, cap = b.transcript_slots()
        mis = [int((int(off[k]) + int(cap[k]) - len(t)) & 3) for k, t in enumerate(txs)]     # the first op's byte in its dword
        assert set(mis) == {0, 1, 2, 3}, mis
        assert any(t.startswith('I') for t in txs) and any(t.startswith('D') for t in txs) and any(t.endswith('I') for t in txs)
        assert any('ID' in t for t in txs)
        # an I run with a 256-byte step of the scan strictly inside it: ONE event
        assert any(s < 256 - mk < e for t, mk in zip(txs, mis) for s, e in _gap_runs(t, 'I')), (mis, [_gap_runs(t, 'I') for t in txs])
        # run boundaries on both sides of a dword and of a 256-byte step
        starts = {(mk + s) & 3 for t, mk in zip(txs, mis) for op in 'ID' for s, _ in _gap_runs(t, op)}
        ends = {(mk + e) & 3 for t, mk in zip(txs, mis) for op in 'ID' for _, e in _gap_runs(t, op)}
        assert starts == {0, 1, 2, 3} and ends == {0, 1, 2, 3}, (starts, ends)
        edges = {(mk + x) - 256 for t, mk in zip(txs, mis) for op in 'ID' for run in _gap_runs(t, op) for x in run}
        assert any(-4 <= d < 0 for d in edges) and any(0 <= d < 4 for d in edges), sorted(edges)
        b.pileup_add(p)
        b.sync()
        got, want = p.counts(), _expected(b, res, txs, p.n_cols, 4)
        assert want[:, 5].sum() == sum(len(_gap_runs(t, 'I')) for t in txs if not t.startswith('I')) + \
            sum(len(_gap_runs(t, 'I')) - 1 for t in txs if t.startswith('I'))
        assert (got == want).all(), np.argwhere(got != want)[:8]


@pytest.fixture(scope='module')
def small():
    """Two small batches over one arena of 13 reads: pairs (0, 1 + k) and pairs (7 + k, 1 + k)."""
    from biseqt_amd import synth
    from biseqt_amd.batch import pack_reads
    rng = synth.rng_for(7303)
    rs = [synth.rand_seqs(rng, 1, 90)[0]]
    rs += [synth.mutate(rng, rs[0][5 * k:5 * k + 50], 0.08, 0.04, 0.4) for k in range(6)]
    rs += [synth.mutate(rng, rs[1 + k], 0.08, 0.04, 0.4) for k in range(6)]
    arena, offs, lens = pack_reads(rs)
    return arena, offs, lens, np.array([(0, 1 + k) for k in range(6)], np.int64), np.array([(7 + k, 1 + k) for k in range(6)], np.int64)


def test_col0_cumulative_adds_and_clear(small):
    from biseqt_amd.batch import BatchAligner, Pileup
    arena, offs, lens, pa, pb = small
    n_cols = arena.nbytes
    kw = dict(alnmode=0, alntype=0, alphabet_len=4, **SCORES)
    with BatchAligner.from_arena(arena, offs, lens, pa, **kw) as a, BatchAligner.from_arena(arena, offs, lens, pb, **kw) as b:
        ra, rb = a.run(), b.run()
        ta, tb = a.transcripts(ra), b.transcripts(rb)
        want_a, want_b = _expected(a, ra, ta, n_cols, 4), _expected(b, rb, tb, n_cols, 4)
        assert want_a.any() and want_b.any() and (want_a != want_b).any()
        with Pileup(n_cols, 4) as p, Pileup(n_cols, 4) as q:
            assert p.counts().shape == (n_cols, 6) and not p.counts().any()             # zeroed at creation
            a.pileup_add(p); a.sync()
            one = p.counts()
            assert (one == want_a).all()
            a.pileup_add(q, col0=offs[pa[:, 0]]); a.sync()                              # the explicit array equals the default
            assert (q.counts() == one).all()                                            # ... and the same add twice is identical
            assert (p.counts(10, 40) == one[10:40]).all() and p.counts(7, 7).shape == (0, 6)
            a.pileup_add(p); a.sync()
            assert (p.counts() == 2 * one).all()                                        # two adds: exactly twice
            b.pileup_add(p); b.sync()
            assert (p.counts() == 2 * want_a + want_b).all()                            # several batches into one pileup
            p.clear(); a.sync()
            assert not p.counts().any()
            b.pileup_add(p); a.pileup_add(p); a.sync(); b.sync()
            assert (p.counts() == want_a + want_b).all()
            # -1 skips its pair; an arena_first moves every frame
            col0 = offs[pb[:, 0]].copy()
            col0[[1, 4]] = -1
            q.clear()
            b.pileup_add(q, col0=col0); b.sync()
            assert (q.counts() == _expected(b, rb, tb, n_cols, 4, col0=[None if c < 0 else c for c in col0])).all()
            assert (q.counts() != want_b).any()
        first = int(offs[7])
        with Pileup(n_cols - first, 4) as p:
            b.pileup_add(p, arena_first=first); b.sync()
            assert (p.counts() == want_b[first:]).all() and p.counts().any()
            p.clear()
            a.pileup_add(p, arena_first=first); a.sync()                                # read 0 lies in front of arena_first: nothing
            assert not p.counts().any()


def test_a_frame_that_overhangs_by_one_column_adds_nothing(small):
    from biseqt_amd.batch import BatchAligner, Pileup
    arena, offs, lens, pa, _ = small
    X = int(lens[0])
    with BatchAligner.from_arena(arena, offs, lens, pa, alnmode=0, alntype=1, alphabet_len=4, **SCORES) as a:
        res = a.run()
        txs = a.transcripts(res)
        assert all(txs)
        # pair 0 fits flush with the end, pair 1 overhangs by ONE column (its local alignment itself would fit), the others
        # are skipped
        col0 = np.array([10, 11, -1, -1, -1, -1], np.int64)
        with Pileup(10 + X, 4) as p:
            a.pileup_add(p, col0=col0); a.sync()
            want = _expected(a, res, txs, 10 + X, 4, col0=[10, None, None, None, None, None])
            assert int(res['origin_idx'][1]) + sum(txs[1].count(c) for c in 'MSD') < X           # the ops alone would fit
            assert (p.counts() == want).all() and want.any()
            last = p.counts(10 + X - 1, 10 + X)
            a.pileup_add(p, col0=np.array([-1, 11, -1, -1, -1, -1], np.int64)); a.sync()
            assert (p.counts() == want).all() and (p.counts(10 + X - 1, 10 + X) == last).all()   # the last column as it was


def test_smaller_alphabet(reads):
    """alphabet_len = 2 over a 4-letter batch: letters 2 and 3 land in no channel, DEL and INS stay at channels 2 and 3."""
    from biseqt_amd.batch import BatchAligner, Pileup
    arena, offs, lens, pairs = reads
    with BatchAligner.from_arena(arena, offs, lens, pairs, alnmode=0, alntype=0, alphabet_len=4, **SCORES) as b, \
            Pileup(300, 2) as p2, Pileup(300, 4) as p4:
        res = b.run()
        txs = b.transcripts(res)
        b.pileup_add(p2); b.pileup_add(p4); b.sync()
        c2, c4 = p2.counts(), p4.counts()
        assert c2.shape == (300, 4)
        assert (c2 == _expected(b, res, txs, 300, 2)).all()
        assert c4[:, 2:4].any()                                     # letters 2 and 3 are there
        assert (c2[:, :2] == c4[:, :2]).all() and (c2[:, 2] == c4[:, 4]).all() and (c2[:, 3] == c4[:, 5]).all()


def test_strip_pipeline_batch():
    from biseqt_amd import _pwlib as W
    from biseqt_amd import synth
    from biseqt_amd.batch import BatchAligner, Pileup
    rng = synth.rng_for(7304)
    pairs = []
    for n in (6000, 300, 1200):
        o = synth.rand_seqs(rng, 1, n)[0]
        pairs.append((o, synth.mutate(rng, o, 0.08, 0.04, 0.3)))
    with BatchAligner(pairs, alnmode=0, alntype=0, alphabet_len=4, flags=W.PW_FLAG_FORCE_STRIP, **SCORES) as b, \
            Pileup(b.arena.nbytes, 4) as p:
        res = b.run()
        txs = b.transcripts(res)
        assert len(txs[0]) >= 6000
        b.pileup_add(p); b.sync()
        got, want = p.counts(), _expected(b, res, txs, p.n_cols, 4)
        assert want[:, :5].sum() == 7500 and (got == want).all(), np.argwhere(got != want)[:8]


def test_pileup_after_traceback_from_explicit_ends():
    """The standard-mode case of tests/test_explicit_ends.py: one problem, every recorded end cell a pair of the batch.  A
    fresh pileup after traceback_from follows the new transcripts."""
    from biseqt_amd.batch import BatchAligner, Pileup
    recs = [r for r in load_golden('explicit_ends.json.gz') if r['kw']['mode'] == 0 and 'origin_range' not in r['kw']][:4]
    for rec in recs:
        kw = kw_of(rec)
        ends = [e['end'] for e in rec['ends']]
        o, m = np.array(dec(rec['origin']), np.uint8), np.array(dec(rec['mutant']), np.uint8)
        with BatchAligner([(o, m)] * len(ends), alnmode=0, alntype=kw['alntype'], alphabet_len=4, subst_scores=kw['subst'],
                          go_score=kw['go'], ge_score=kw['ge']) as b:
            n_cols = b.arena.nbytes
            res0 = b.run()
            txs0 = b.transcripts(res0)
            with Pileup(n_cols, 4) as p:
                b.pileup_add(p); b.sync()
                first = p.counts()
                assert (first == _expected(b, res0, txs0, n_cols, 4)).all()
            b.traceback_from(ends)
            b.sync()
            res = b.results()
            txs = b.transcripts(res)
            assert txs != txs0
            with Pileup(n_cols, 4) as p:
                b.pileup_add(p); b.sync()
                assert (p.counts() == _expected(b, res, txs, n_cols, 4)).all() and (p.counts() != first).any()


def test_refusals():
    from biseqt_amd import _pwlib as W
    from biseqt_amd import synth
    from biseqt_amd.batch import BatchAligner, Pileup
    lib = W.load()
    for L in (0, 33):
        assert not lib.pw_pileup_create(0, 100, L) and 'alphabet_len must be 1..32' in W.last_error()
        with pytest.raises(ValueError):
            Pileup(100, L)
    origins, mutants = synth.pair_batch(12, 60, 61)
    with BatchAligner(list(zip(origins, mutants)), alnmode=0, alntype=0, alphabet_len=4, **SCORES) as b, \
            Pileup(b.arena.nbytes, 4) as p, Pileup(8, 32) as wide:
        with pytest.raises(RuntimeError, match='before a traceback'):
            b.pileup_add(p)
        b.solve()
        with pytest.raises(RuntimeError, match='before a traceback'):
            b.pileup_add(p)
        with pytest.raises(ValueError):
            b.pileup_add(p, col0=np.zeros(b.n + 1, np.int64))
        with pytest.raises(ValueError):
            b.pileup_add(object())
        b.sync()
        assert not p.counts().any()
        with pytest.raises(RuntimeError, match='before pw_pileup_call'):
            p.sites()
        with pytest.raises(RuntimeError, match='before call'):
            p.sites_device()
        for lo, hi in ((-1, 2), (3, 2), (0, p.n_cols + 1)):
            with pytest.raises(ValueError):
                p.counts(lo, hi)
        out = np.zeros(6, np.uint32)
        assert lib.pw_pileup_counts(p.handle, 0, p.n_cols + 1, out.ctypes.data) == -1 and 'outside the pileup' in W.last_error()
        b.traceback()
        b.pileup_add(p); b.pileup_add(wide); b.sync()             # every frame lies outside the 8 columns of `wide`
        assert p.counts().any() and wide.counts().shape == (8, 34) and not wide.counts().any()
        assert p.counts_device().ptr and p.counts_device().nbytes == 4 * 6 * p.n_cols


def _hand_counts(n_cols, L, seed):
    """Random small counts (ties and empty columns abound) with constructed columns in front, as many as fit: the two top
    letters tie, DEL wins, 2 * INS == depth (no flag), 2 * INS == depth + 1 (flag), an empty column, a deep one."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 4, size=(n_cols, L + 2)).astype(np.uint32)
    special = np.array([[0, 5, 5, 1, 2, 0], [1, 0, 2, 0, 4, 1], [2, 0, 1, 1, 0, 2], [2, 0, 0, 0, 1, 2], [0, 0, 0, 0, 0, 3],
                        [4000000000, 1, 0, 0, 3, 2000000003]], np.uint32)
    k = min(n_cols, len(special))
    c[:k] = special[:k]
    return c


@pytest.mark.parametrize('n_cols', (1, 63, 64, 65, 300))
def test_call_against_the_numpy_oracle(global_counts, n_cols):
    from biseqt_amd.batch import DeviceArena, Pileup, SITE_DTYPE
    from biseqt_amd import _pwlib as W
    L = 4
    tables = [_hand_counts(n_cols, L, 7400 + n_cols)] + ([global_counts] if n_cols == 300 else [])
    rng = np.random.default_rng(7500 + n_cols)
    ref = rng.integers(0, L, n_cols).astype(np.uint8)
    host = np.concatenate([np.full(16, 9, np.uint8), ref, np.full(16, 9, np.uint8)])
    with Pileup(n_cols, L) as p, DeviceArena(host) as dref:
        for counts in tables:
            p.set_counts(counts)
            assert (p.counts() == counts).all()
            for min_depth in (1, 3):
                for given, want_ref in ((None, None), (ref, ref), ((dref, 16), ref)):
                    p.call(given, min_depth=min_depth)
                    got, want = p.sites(), R.call(counts, L, want_ref, min_depth)
                    assert got.dtype == SITE_DTYPE
                    for f in ('depth', 'call', 'ref', 'flags'):
                        assert (got[f] == want[f]).all(), (f, min_depth, np.flatnonzero(got[f] != want[f])[:8])
                    assert (p.consensus() == want['call']).all()
                    lo, hi = n_cols // 3, n_cols
                    assert (p.sites(lo, hi) == got[lo:hi]).all() and (p.consensus(lo, hi) == want['call'][lo:hi]).all()
                    flagged = np.flatnonzero(want['flags'] & (W.PW_PILEUP_DIFFERS | W.PW_PILEUP_INSERT))
                    assert p.variants().tolist() == flagged.tolist()
                    assert p.variants(lo, hi).tolist() == [c for c in flagged.tolist() if lo <= c < hi]
            assert p.sites_device().ptr and p.sites_device().nbytes == 8 * n_cols
        # the constructed columns say what they were built for (the numpy oracle is checked on its own in test_pileup_ref.py)
        want = R.call(tables[0], L, None, 1)
        if n_cols >= 5:
            assert [int(x) for x in want['call'][:5]] == [1, L, 0, 0, 255]
            assert [int(x) & W.PW_PILEUP_INSERT for x in want['flags'][:5]] == [0, 0, 0, 4, 0] and int(want['depth'][2]) == 4
        with pytest.raises(ValueError):
            p.call(ref[:-1] if n_cols > 1 else np.zeros(2, np.uint8))
        with pytest.raises(ValueError):
            p.call((dref, len(host) - n_cols + 1))
