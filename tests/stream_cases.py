"""The cases of tests/test_gpu_streams.py: probe batches whose letters exist in several arenas of ONE geometry, so that a
handle can be filled with the answers of one arena (the poison) and then asked, on a busy non-default stream, for those of
another -- a stale read, a missing wait or a launch on the wrong stream then shows in whatever field a test compares.

A probe batch is built like the fixtures of tests/test_gpu_cigar_batch.py: mutated copies of random origins, and every
eighth pair with no letter in common.  All arenas of a case share the lengths of every pair (hence frame offsets, slots and
table shapes); the letters differ, the pair without a common letter sits at another residue of 8 in every arena (so no pair
lacks an alignment in two arenas), and the gap rate grows with the arena index (so the packed offsets drift apart); the
seed is one at which all of that holds.  tests/test_stream_cases.py proves from the oracle alone that every pair and every
packed offset differs between arenas.

Everything expected comes from the CPU oracle and the pure-Python references applied to the oracle's transcripts."""
import numpy as np

from tests import cigar_ref, pileup_ref, tx_summary_ref

SCORES = dict(match_score=1, mismatch_score=-3, go_score=-5, ge_score=-2)
OSCORES = dict(match=1, mismatch=-3, go=-5, ge=-2, L=4)
ARENAS = 3                                   # 0: Y, the arena under test; 1: X', the poison; 2: the third of the ring
GAP_RATES = (0.02, 0.04, 0.06)
BAND = (-25, 25)
# name -> (alnmode, alntype): GLOBAL, LOCAL and OVERLAP in standard mode, B_LOCAL in banded mode
TYPES = {'global': (0, 0), 'local': (0, 1), 'overlap': (0, 4), 'b_local': (1, 1)}
PROBE = dict(seed=5103, n=64, lo=60, hi=300)
# the front load: pairs of 1000 letters, banded +-100, f64.  FRONT_PAIRS is sized on the MI355X (profiles/streams_probe.txt);
# the pairs are FRONT_DISTINCT different ones, repeated (their letters are not the subject, their device time is)
FRONT_PAIRS, FRONT_DISTINCT = 32000, 4000
FRONT_LEN, FRONT_BAND = 1000, (-100, 100)
# the kernel-family cases that need another shape than the probe batch: family -> (type, case, band, no_common)
FAMILY_CASES = {
    'fill16-mw': ('b_local', dict(seed=5201, n=8, lo=690, hi=700), (-500, 500), False),
    'tiled': ('global', dict(seed=5202, n=1, lo=1200, hi=1200), BAND, False),
    'strip': ('global', dict(seed=5203, n=1, lo=6000, hi=6000), BAND, False),
}


def geometry(seed, n, lo, hi):
    """``[(X, Y)]``: the lengths of the n pairs of a case, shared by all its arenas."""
    rng = np.random.Generator(np.random.PCG64(seed))
    xs = rng.integers(lo, hi + 1, size=n)
    return [(int(x), int(x) - int(t)) for x, t in zip(xs, rng.integers(0, 9, size=n))]


def pairs_of(arena, seed, n, lo, hi, no_common=True):
    """The n ``(origin, mutant)`` pairs of arena ``arena`` of the case ``(seed, n, lo, hi)``."""
    from biseqt_amd import synth
    rng = synth.rng_for(1000 * seed + arena)
    out = []
    for k, (X, Y) in enumerate(geometry(seed, n, lo, hi)):
        o = synth.rand_seqs(rng, 1, X)[0]
        if no_common and k % 8 == 7 - arena:
            o = (o % 2).astype(np.uint8)
            out.append((o, ((o + 2) % 4)[:Y].astype(np.uint8)))
            continue
        m = synth.mutate(rng, o, 0.08, GAP_RATES[arena], 0.4)
        m = np.concatenate([m, synth.rand_seqs(rng, 1, Y)[0]])[:Y].astype(np.uint8)      # the geometry's length exactly
        out.append((o, m))
    return out


def probe_pairs(arena):
    return pairs_of(arena, **PROBE)


def layout(pairs):
    """``(arena bytes, [(origin_off, mutant_off)])`` as ``BatchAligner`` lays its pairs out: every sequence on a 16-byte
    boundary with 16 bytes of slack (the GPU tests assert that this equals the batch's own arena)."""
    offs, total = [], 0
    for o, m in pairs:
        oo = total
        total += (len(o) + 15) // 16 * 16 + 16
        mo = total
        total += (len(m) + 15) // 16 * 16 + 16
        offs.append((oo, mo))
    arena = np.zeros(max(total, 16), np.uint8)
    for (o, m), (oo, mo) in zip(pairs, offs):
        arena[oo:oo + len(o)] = o
        arena[mo:mo + len(m)] = m
    return arena, offs


def batch_kw(name, band=BAND):
    mode, alntype = TYPES[name]
    kw = dict(alnmode=mode, alntype=alntype, alphabet_len=4, **SCORES)
    if mode == 1:
        kw.update(diag_range=band, check_band=False)
    return kw


def oracle_kw(name, band=BAND):
    mode, alntype = TYPES[name]
    kw = dict(mode=mode, alntype=alntype, **OSCORES)
    if mode == 1:
        kw['diag_range'] = band
    return kw


REC_DTYPE = np.dtype([('origin_idx', '<i4'), ('mutant_idx', '<i4'), ('status', '<i4')])


class Expected(object):
    """What the oracle says about the pairs of one arena under one alignment type.

    ``view``: per pair ``(end cell, score, tb_null, transcript, start)`` -- only the end cell where the table has none, no
    start without a transcript; ``txs`` the transcripts (None without one); ``packed`` their concatenation and its
    offsets; ``summaries`` / ``cigars[form]`` / ``pileup(...)`` the pure-Python references applied to ``txs``."""

    def __init__(self, oracle, pairs, name, band=BAND):
        self.pairs, self.name = pairs, name
        self.raw = [oracle.solve(o, m, **oracle_kw(name, band)) for o, m in pairs]
        self.view, self.txs = [], []
        self.rec = np.zeros(len(pairs), REC_DTYPE)
        for k, r in enumerate(self.raw):
            assert r['init_rc'] == 0, (name, k)
            if r['opt'][0] == -1:
                self.view.append((r['opt'], None, None, None, None))
                self.txs.append(None)
                continue
            assert not r['would_panick'], (name, k)
            tx = r['transcript'] or None
            self.view.append((r['opt'], float(r['score']), bool(r['tb_null']), tx,
                              (r['origin_idx'], r['mutant_idx']) if tx else None))
            self.txs.append(tx)
            if tx:
                self.rec[k] = (r['origin_idx'], r['mutant_idx'], pileup_ref.ST_TRACED)
        raw = [(t or '').encode('ascii') for t in self.txs]
        self.packed_offsets = np.zeros(len(raw) + 1, np.uint64)
        self.packed_offsets[1:] = np.cumsum([len(r) for r in raw])
        self.packed_bytes = np.frombuffer(b''.join(raw), np.uint8)
        self.summaries = [tx_summary_ref.summarize(t) for t in self.txs]
        self.cigars = {nm: cigar_ref.packed(self.txs, form) for nm, form in cigar_ref.FORMS}
        self.ends = np.array([r['opt'] for r in self.raw], np.int32).reshape(len(pairs), 2)

    def pileup(self, n_cols, col0=None):
        """The oracle's pileup of the batch: origin frames at their arena offsets, or at ``col0`` (negative: skipped)."""
        offs = layout(self.pairs)[1]
        frames = [oo for oo, _ in offs] if col0 is None else [None if c < 0 else int(c) for c in col0]
        return pileup_ref.of_batch(n_cols, 4, self.rec, self.txs, frames, [m for _, m in self.pairs],
                                   [len(o) for o, _ in self.pairs])


_EXPECTED = {}


def expected(oracle, arena, name, case=None, band=BAND, no_common=True):
    """``Expected`` of arena ``arena`` of a case (default: the probe batch), computed once per process and left unchanged."""
    case = dict(PROBE) if case is None else case
    key = (arena, name, tuple(sorted(case.items())), band, no_common)
    if key not in _EXPECTED:
        _EXPECTED[key] = Expected(oracle, pairs_of(arena, no_common=no_common, **case), name, band)
    return _EXPECTED[key]


def view_of(res, txs):
    """The records and transcripts of a batch in the form of ``Expected.view``."""
    out = []
    for k in range(len(res)):
        opt = (int(res['opt_i'][k]), int(res['opt_j'][k]))
        if opt[0] == -1:
            out.append((opt, None, None, None, None))
            continue
        st = int(res['status'][k])
        assert st & 1 and not st & 12, (k, st)                         # traced; no panick, no bad path
        tx = txs[k] or None
        out.append((opt, float(res['score'][k]), bool(st & 2), tx,
                    (int(res['origin_idx'][k]), int(res['mutant_idx'][k])) if tx else None))
    return out


_FRONT = []


def front_pairs(n=None):
    from biseqt_amd import synth
    n = FRONT_PAIRS if n is None else n
    if not _FRONT:
        _FRONT.extend(zip(*synth.pair_batch(5200, FRONT_DISTINCT, FRONT_LEN)))
    return [_FRONT[k % FRONT_DISTINCT] for k in range(n)]
