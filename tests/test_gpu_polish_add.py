"""The two-sided pileups with insertion slots (``BatchAligner.pileup_add(sides=...)``; include/pw_polish.h) against the oracle
of tests/polish_ref.py applied to ``b.transcripts(res)`` and ``res`` of the same batch: every comparison is ``==`` on integer
counts.  Colliding wavefronts on both reads' columns, the edges of the kernel's dword, lane and pass scan, reversed pairs,
frames, cumulative adds, a smaller alphabet, the strip pipeline, and the old entry point."""
import numpy as np
import pytest

from tests import polish_add_cases as AC
from tests import polish_ref as PR

pytestmark = pytest.mark.gpu

SCORES = dict(match_score=1, mismatch_score=-3, go_score=-5, ge_score=-2)
COMP = np.array([3, 2, 1, 0], np.uint8)


def _geo_arena(b):
    """geo of a batch whose letters are all in its host arena."""
    p = b._pairs
    rows = ([(int(r['origin_off']), int(r['mutant_off']), int(r['origin_len']), int(r['mutant_len'])) for r in p[:b.n]]
            if isinstance(p, np.ndarray) else
            [(int(p[k].origin_off), int(p[k].mutant_off), int(p[k].origin_len), int(p[k].mutant_len)) for k in range(b.n)])
    return [(oo, mo, b.arena[oo:oo + X], b.arena[mo:mo + Y]) for oo, mo, X, Y in rows]


def _same(pile, want, J):
    """The device's counts and plane against the oracle's (computed with at least J slots: a plane of fewer slots is the
    first ones of a larger plane)."""
    got = pile.counts()
    assert (got == want[0]).all(), np.argwhere(got != want[0])[:8]
    if J:
        gi = pile.ins_counts()
        assert gi.shape == (pile.n_cols, J, pile.alphabet_len)
        assert (gi == want[1][:, :J]).all(), np.argwhere(gi != want[1][:, :J])[:8]


@pytest.fixture(scope='module')
def reads():
    """One 300-letter origin and 64 windows of it, mutated; pairs (0, 1 + k) for even k and (1 + k, 0) for odd k: the
    wavefronts collide on read 0's columns from the origin side AND from the mutant side."""
    from biseqt_amd import synth
    from biseqt_amd.batch import pack_reads
    rng = synth.rng_for(7702)
    origin = synth.rand_seqs(rng, 1, 300)[0]
    rs = [origin]
    for k in range(64):
        n = int(rng.integers(285, 301)) if k % 4 < 2 else int(rng.integers(60, 201))
        s = int(rng.integers(0, 300 - n + 1))
        rs.append(synth.mutate(rng, origin[s:s + n], 0.08, 0.05, 0.5))
    arena, offs, lens = pack_reads(rs)
    return arena, offs, lens, np.array([(0, 1 + k) if k % 2 == 0 else (1 + k, 0) for k in range(64)], np.int64)


@pytest.mark.parametrize('mode,alntype', [(1, 2), (1, 1), (0, 0), (0, 4)], ids=['B_OVERLAP', 'B_LOCAL', 'GLOBAL', 'OVERLAP'])
def test_colliding_windows_every_side_and_slot_count(reads, mode, alntype):
    from biseqt_amd.batch import BatchAligner, Pileup
    arena, offs, lens, pairs = reads
    kw = dict(diag_ranges=[(-25, 25)] * len(pairs), check_band=False) if mode == 1 else {}
    n_cols = arena.nbytes
    with BatchAligner.from_arena(arena, offs, lens, pairs, alnmode=mode, alntype=alntype, alphabet_len=4, **SCORES, **kw) as b:
        res = b.run()
        txs = b.transcripts(res)
        assert sum(1 for t in txs if t) >= 20
        geo = _geo_arena(b)
        want = {s: AC.expected(n_cols, 4, 8, res, txs, geo, s) for s in (1, 2)}
        want[3] = (want[1][0] + want[2][0], want[1][1] + want[2][1])
        lo, hi = int(offs[0]), int(offs[0]) + 300
        assert want[1][0][lo:hi].max() >= 8 and want[2][0][lo:hi].max() >= 8        # both sides do collide on read 0
        assert want[3][1][:, 0].any() and want[3][1][:, 1].any()                     # runs of two and more are there
        for sides, name in ((1, 'origin'), (2, 'mutant'), (3, 'both')):
            for J in (0, 1, 2, 8):
                with Pileup(n_cols, 4, ins_slots=J) as p:
                    b.pileup_add(p, sides=name, mutant_col0=None if J else offs[pairs[:, 1]])   # explicit == default
                    b.sync()
                    _same(p, want[sides], J)


def test_transcript_lengths_and_runs_across_dword_lane_and_pass_edges():
    from biseqt_amd.batch import BatchAligner, Pileup
    pairs = AC.scan_pairs()
    with BatchAligner(pairs, alnmode=0, alntype=0, alphabet_len=4, **AC.GAPPY) as b:
        res = b.run()
        txs = b.transcripts(res)
        assert all(txs) and set(AC.SCAN_LENGTHS) <= {len(t) for t in txs}
        off, cap = b.transcript_slots()
        mis = [int((int(off[k]) + int(cap[k]) - len(t)) & 3) for k, t in enumerate(txs)]       # the first op's byte in its dword
        assert set(mis) == {0, 1, 2, 3}, mis
        for op in 'ID':
            assert any(t.startswith(op) for t in txs) and any(t.endswith(op) for t in txs)
            runs = [(len(t), mk, s, e) for t, mk in zip(txs, mis) for s, e in AC.gap_runs(t, op)]
            assert {e - s for _, _, s, e in runs} >= set(AC.RUN_LENGTHS)
            # forward stream (op k in byte mis + k) and reversed stream (op n - 1 - k in byte 4 * nq - mis - n + k)
            for fwd in (True, False):
                at = [(mk + s, mk + e) if fwd else (4 * ((mk + n + 3) >> 2) - mk - e, 4 * ((mk + n + 3) >> 2) - mk - s) for n, mk, s, e in runs]
                assert {s & 3 for s, _ in at} == {0, 1, 2, 3} and {e & 3 for _, e in at} == {0, 1, 2, 3}
                assert any(s < 256 < e for s, e in at), 'no run straddles a pass edge'
                assert any(e - s >= 3 and (s >> 2) != ((e - 1) >> 2) for s, e in at)             # ... a dword = lane edge
        assert any('ID' in t or 'DI' in t for t in txs)                                          # a run directly behind the other kind
        geo = _geo_arena(b)
        n_cols = b.arena.nbytes
        want = {s: AC.expected(n_cols, 4, 8, res, txs, geo, s) for s in (1, 2)}
        want[3] = (want[1][0] + want[2][0], want[1][1] + want[2][1])
        assert want[3][1][:, 7].any()                                                            # runs of eight and more
        rev = np.ones(b.n, np.uint8)
        want_rev = AC.expected(n_cols, 4, 8, res, txs, geo, 2, rev=rev, comp=COMP)
        for J in (2, 8):
            with Pileup(n_cols, 4, ins_slots=J) as p:
                b.pileup_add(p, sides='both'); b.sync()
                _same(p, want[3], J)
                p.clear()
                b.pileup_add(p, sides='mutant', reverse=rev, complement=COMP); b.sync()          # the same transcripts from their last op
                _same(p, want_rev, J)
                assert (p.counts() != want[2][0]).any()


@pytest.fixture(scope='module')
def stranded():
    """Six reads; pairs with the forward read 0 as origin: three forward mutants and three whose READ is the reverse complement
    of a window of read 0 (the batch aligns read 0 with rc(read) behind the arena)."""
    from biseqt_amd import synth
    from biseqt_amd.batch import pack_reads
    rng = synth.rng_for(7703)
    origin = synth.rand_seqs(rng, 1, 240)[0]
    rs = [origin]
    for k in range(6):
        w = synth.mutate(rng, origin[20 * k:20 * k + 120], 0.06, 0.05, 0.5)
        rs.append(COMP[w[::-1]] if k % 2 else w)
    arena, offs, lens = pack_reads(rs)
    pairs = np.array([(0, 1 + k) for k in range(6)], np.int64)
    return rs, arena, offs, lens, pairs, np.array([k % 2 for k in range(6)], np.uint8)


def test_reversed_pairs_mixed_with_forward_pairs(stranded):
    from biseqt_amd.batch import BatchAligner, DeviceArena, Pileup
    rs, arena, offs, lens, pairs, minus = stranded
    which = np.unique(pairs[minus == 1, 1])
    n_cols = arena.nbytes
    with DeviceArena.with_reverse_complements(arena, offs, lens, which, COMP) as dev:
        all_offs = np.concatenate([offs, dev.rc_offsets])
        all_lens = np.concatenate([lens, lens[which]])
        pidx = pairs.copy()
        pidx[minus == 1, 1] = len(offs) + np.searchsorted(which, pairs[minus == 1, 1])
        with BatchAligner.from_arena(arena, all_offs, all_lens, pidx, [(-120, 240)] * 6, device_arena=dev, alnmode=1, alntype=2,
                                     alphabet_len=4, arena_bytes=dev.nbytes, check_band=False, **SCORES) as b:
            res = b.run()
            txs = b.transcripts(res)
            assert all(txs) and all(len(t) >= 60 for t in txs)
            geo = [(int(offs[0]), int(all_offs[pidx[k, 1]]), rs[0], COMP[rs[1 + k][::-1]] if minus[k] else rs[1 + k]) for k in range(6)]
            mcol0 = offs[pairs[:, 1]]
            want = AC.expected(n_cols, 4, 2, res, txs, geo, 3, mcol0=mcol0, rev=minus, comp=COMP)
            assert want[1].any() and any(want[0][int(offs[1 + k]):int(offs[1 + k]) + int(lens[1 + k]), :4].any() for k in (1, 3, 5))
            with Pileup(n_cols, 4, ins_slots=2) as p:
                b.pileup_add(p, sides='both', mutant_col0=mcol0, reverse=minus, complement=COMP); b.sync()
                _same(p, want, 2)
                # the forward letters of a reversed read agree with what is piled onto them: the calls follow the read
                for k in (1, 3, 5):
                    lo = int(offs[1 + k])
                    cols = p.counts(lo, lo + int(lens[1 + k]))[:, :4]
                    seen = cols.sum(axis=1) > 0
                    assert seen.sum() >= 80 and (cols.argmax(axis=1)[seen] == rs[1 + k][seen]).mean() > .8
                # without mutant_col0 the rc frames lie behind the pileup: the mutant side of the minus pairs adds nothing
                p.clear()
                b.pileup_add(p, sides='mutant', reverse=minus, complement=COMP); b.sync()
                _same(p, AC.expected(n_cols, 4, 2, res, txs, geo, 2, rev=minus, comp=COMP), 2)
            with pytest.raises(RuntimeError, match='complement'):
                with Pileup(n_cols, 4) as p:
                    b.pileup_add(p, sides='both', reverse=minus, complement=np.array([1, 0, 2, 2], np.uint8))


@pytest.fixture(scope='module')
def small():
    """Two small batches over one arena of 13 reads: pairs (0, 1 + k) and pairs (7 + k, 1 + k)."""
    from biseqt_amd import synth
    from biseqt_amd.batch import pack_reads
    rng = synth.rng_for(7704)
    rs = [synth.rand_seqs(rng, 1, 90)[0]]
    rs += [synth.mutate(rng, rs[0][5 * k:5 * k + 50], 0.08, 0.05, 0.5) for k in range(6)]
    rs += [synth.mutate(rng, rs[1 + k], 0.08, 0.05, 0.5) for k in range(6)]
    arena, offs, lens = pack_reads(rs)
    return arena, offs, lens, np.array([(0, 1 + k) for k in range(6)], np.int64), np.array([(7 + k, 1 + k) for k in range(6)], np.int64)


def test_frames_cumulative_adds_and_clear(small):
    from biseqt_amd.batch import BatchAligner, Pileup
    arena, offs, lens, pa, pb = small
    n_cols = arena.nbytes
    kw = dict(alnmode=0, alntype=0, alphabet_len=4, **SCORES)
    with BatchAligner.from_arena(arena, offs, lens, pa, **kw) as a, BatchAligner.from_arena(arena, offs, lens, pb, **kw) as b:
        ra, rb = a.run(), b.run()
        ta, tb = a.transcripts(ra), b.transcripts(rb)
        ga, gb = _geo_arena(a), _geo_arena(b)
        wa, wb = AC.expected(n_cols, 4, 2, ra, ta, ga, 3), AC.expected(n_cols, 4, 2, rb, tb, gb, 3)
        assert wa[1].any() and wb[1].any()
        with Pileup(n_cols, 4, ins_slots=2) as p, Pileup(n_cols, 4, ins_slots=2) as q:
            assert p.ins_counts().shape == (n_cols, 2, 4) and not p.ins_counts().any() and p.ins_counts(3, 3).shape == (0, 2, 4)
            a.pileup_add(p, sides='both'); a.sync()
            _same(p, wa, 2)
            a.pileup_add(q, sides='both', col0=offs[pa[:, 0]], mutant_col0=offs[pa[:, 1]]); a.sync()   # explicit == default
            _same(q, wa, 2)
            assert (p.ins_counts(10, 40) == wa[1][10:40]).all()
            a.pileup_add(p, sides='both'); a.sync()
            _same(p, (2 * wa[0], 2 * wa[1]), 2)                                                   # two adds: exactly twice
            b.pileup_add(p, sides='both'); b.sync()
            _same(p, (2 * wa[0] + wb[0], 2 * wa[1] + wb[1]), 2)                                   # two batches into one pileup
            p.clear(); a.sync()
            assert not p.counts().any() and not p.ins_counts().any()                              # clear zeroes the plane too
            b.pileup_add(p, sides='both'); a.pileup_add(p, sides='both'); a.sync(); b.sync()
            _same(p, (wa[0] + wb[0], wa[1] + wb[1]), 2)
            # -1 skips that side of its pair only
            oc, mc = offs[pb[:, 0]].copy(), offs[pb[:, 1]].copy()
            oc[[1, 4]] = -1
            mc[[0, 4]] = -1
            q.clear()
            b.pileup_add(q, sides='both', col0=oc, mutant_col0=mc); b.sync()
            _same(q, AC.expected(n_cols, 4, 2, rb, tb, gb, 3, ocol0=oc, mcol0=mc), 2)
            assert (q.counts() != wb[0]).any()
        first = int(offs[7])
        with Pileup(n_cols - first, 4, ins_slots=2) as p:                                         # arena_first moves every frame
            b.pileup_add(p, sides='both', arena_first=first); b.sync()
            _same(p, AC.expected(n_cols - first, 4, 2, rb, tb, gb, 3, arena_first=first), 2)
            assert p.counts().any() and not p.counts(0, 0).size
        # a mutant frame that overhangs by ONE column adds nothing on that side; flush with the end it fits
        Y0, Y1 = int(lens[1]), int(lens[2])
        n = 20 + Y1                                                                               # pair 1 at column 21 ends one past it
        assert n - Y0 >= 0
        with Pileup(n, 4, ins_slots=2) as p:
            a.pileup_add(p, sides='mutant', mutant_col0=np.array([n - Y0, 21, -1, -1, -1, -1], np.int64)); a.sync()
            want = AC.expected(n, 4, 2, ra, ta, ga, 2, mcol0=[n - Y0, -1, -1, -1, -1, -1])
            assert want[0][n - 1].any()                                                           # the flush frame reaches the last column
            _same(p, want, 2)


def test_smaller_alphabet(reads):
    """alphabet_len = 2 over a 4-letter batch: letters 2 and 3 land in no channel and in no slot."""
    from biseqt_amd.batch import BatchAligner, Pileup
    arena, offs, lens, pairs = reads
    n_cols = arena.nbytes
    with BatchAligner.from_arena(arena, offs, lens, pairs, alnmode=0, alntype=0, alphabet_len=4, **SCORES) as b, \
            Pileup(n_cols, 2, ins_slots=2) as p2, Pileup(n_cols, 4, ins_slots=2) as p4:
        res = b.run()
        txs = b.transcripts(res)
        b.pileup_add(p2, sides='both'); b.pileup_add(p4, sides='both'); b.sync()
        _same(p2, AC.expected(n_cols, 2, 2, res, txs, _geo_arena(b), 3), 2)
        i2, i4 = p2.ins_counts(), p4.ins_counts()
        assert i2.shape == (n_cols, 2, 2) and i4[:, :, 2:].any() and (i2 == i4[:, :, :2]).all()


def test_strip_batch():
    from biseqt_amd import _pwlib as W
    from biseqt_amd import synth
    from biseqt_amd.batch import BatchAligner, Pileup
    rng = synth.rng_for(7705)
    pairs = []
    for n in (6000, 300, 1200):
        o = synth.rand_seqs(rng, 1, n)[0]
        pairs.append((o, synth.mutate(rng, o, 0.08, 0.04, 0.4)))
    with BatchAligner(pairs, alnmode=0, alntype=0, alphabet_len=4, flags=W.PW_FLAG_FORCE_STRIP, **SCORES) as b, \
            Pileup(b.arena.nbytes, 4, ins_slots=2) as p:
        res = b.run()
        txs = b.transcripts(res)
        assert len(txs[0]) >= 6000
        geo = _geo_arena(b)
        b.pileup_add(p, sides='both'); b.sync()
        _same(p, AC.expected(p.n_cols, 4, 2, res, txs, geo, 3), 2)
        p.clear()
        rev = np.array([1, 0, 1], np.uint8)
        b.pileup_add(p, sides='mutant', reverse=rev, complement=COMP); b.sync()                   # a long transcript from its end
        _same(p, AC.expected(p.n_cols, 4, 2, res, txs, geo, 2, rev=rev, comp=COMP), 2)


def test_origin_side_without_a_plane_equals_the_old_entry_point(reads):
    from biseqt_amd import _pwlib as W
    from biseqt_amd.batch import BatchAligner, Pileup
    arena, offs, lens, pairs = reads
    n_cols = arena.nbytes
    lib = W.load()
    with BatchAligner.from_arena(arena, offs, lens, pairs, alnmode=0, alntype=4, alphabet_len=4, **SCORES) as b, \
            Pileup(n_cols, 4) as old, Pileup(n_cols, 4) as new, Pileup(n_cols, 4, ins_slots=3) as plane:
        with pytest.raises(RuntimeError, match='before a traceback'):
            b.pileup_add(new, sides='both')
        b.run()
        b.pileup_add(old)                                                                         # pw_batch_pileup_add
        assert lib.pw_batch_pileup_add_sides(b.handle, new.handle, 1, None, None, None, None, 0, 0, None) == 0
        b.pileup_add(plane, sides='origin', mutant_col0=offs[pairs[:, 1]])                        # ... through pileup_add too
        b.sync()
        assert old.counts().any() and (new.counts() == old.counts()).all() and (plane.counts() == old.counts()).all()
        assert lib.pw_pileup_ins_slots(old.handle) == 0 and lib.pw_pileup_ins_slots(plane.handle) == 3
        assert not lib.pw_pileup_ins_counts_device(old.handle) and lib.pw_pileup_ins_counts_device(plane.handle)
        out = np.zeros(12, np.uint32)
        assert lib.pw_pileup_ins_counts(old.handle, 0, 1, out.ctypes.data) == -1 and 'no insertion plane' in W.last_error()
        for sides in (0, 4):
            assert lib.pw_batch_pileup_add_sides(b.handle, new.handle, sides, None, None, None, None, 0, 0, None) == -1
            assert 'sides must be' in W.last_error()
        rev = np.ones(b.n, np.uint8)
        assert lib.pw_batch_pileup_add_sides(b.handle, new.handle, 3, None, None, rev.ctypes.data, None, 0, 0, None) == -1
        assert 'need a complement' in W.last_error()
        b.sync()
        assert (new.counts() == old.counts()).all()                                               # the refused calls added nothing
