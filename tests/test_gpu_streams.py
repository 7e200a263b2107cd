"""The stream-taking batch surface off the default stream: every entry point that takes a ``void* stream`` is run on
non-blocking torch streams (``torch.cuda.Stream(device=0).cuda_stream``, as bench.py takes them), one and two batches in
flight, and compared with ``==`` against the CPU oracle and the pure-Python references applied to the oracle's transcripts.

The probe pattern.  A missing dependency shows only while the device is still busy when the dependent work is queued, so
every probe (1) queues a front load F first on the stream -- ``SC.FRONT_PAIRS`` pairs of 1000 letters, banded, f64; checked
only against its own default-stream run -- (2) uses a small handle P that was run to completion on the default stream with
a poison arena X' of the same geometry, so that every buffer holds X' answers, and (3) queues the chain under test behind
F, starting with ``upload_async(Y)``, synchronises once at the end and compares everything with the oracle on Y.
tests/test_stream_cases.py proves that X' and Y differ in every pair and every packed offset.  Right behind each critical
call the test reads ``stream.query()``: it must be ``False`` (the device still works), or the probe proved nothing and the
test fails.  Calls that block on their stream by contract (``pw_batch_cigars``, the k-mer and seed builds) are entered
while the stream is busy instead.  profiles/streams_probe.txt has the sizing of F."""
import ctypes
import time

import numpy as np
import pytest

from tests import cigar_ref, kmer_ref as KR, pileup_ref, stream_cases as SC, tx_summary_ref
from tests.plane_checks import check_walks

pytestmark = pytest.mark.gpu

FORMS = dict(cigar_ref.FORMS)


def _streams(n):
    import torch
    assert n <= 3
    return [torch.cuda.Stream(device=0) for _ in range(n)]


def _dev(buf, dtype=np.uint8):
    """The bytes behind a DeviceBuffer view, on the host."""
    import torch
    if not buf.nbytes:
        return np.zeros(0, dtype)
    return torch.as_tensor(buf, device='cuda').cpu().numpy().view(dtype)


def _pinned(values, dtype=np.uint8):
    from biseqt_amd.batch import PinnedArray
    values = np.ascontiguousarray(values, dtype)
    p = PinnedArray(values.nbytes, dtype)
    p.array[:] = values
    return p


class Front(object):
    """The front load F: one handle, solved + traced + packed once on the default stream for reference; ``queue`` puts the
    same work on a stream, ``check`` (after the caller's synchronisation) compares records and packed transcripts."""

    def __init__(self, n=None, flags=0):
        from biseqt_amd import _pwlib as W
        from biseqt_amd.batch import BatchAligner
        self.b = BatchAligner(SC.front_pairs(n), alnmode=1, alntype=1, alphabet_len=4, diag_range=SC.FRONT_BAND,
                              flags=W.PW_FLAG_FORCE_F64 | flags, **SC.SCORES)
        self.b.solve()
        self.b.traceback()
        self.b.pack_transcripts()
        self.b.sync()
        self.res = self.b.results().copy()
        self.packed = [a.copy() for a in self.b.packed()]
        assert (self.res['tx_len'] > 0).all()

    def queue(self, st):
        s = st.cuda_stream
        self.b.solve(s)
        self.b.traceback(s)
        self.b.pack_transcripts(s)

    def check(self):
        assert np.array_equal(self.b.results(), self.res)
        buf, off = self.b.packed()
        assert np.array_equal(off, self.packed[1]) and np.array_equal(buf, self.packed[0])


@pytest.fixture(scope='module')
def front():
    f = Front()
    yield f
    f.b.close()


@pytest.fixture(scope='module')
def front2():
    """A second front load, for the probes that keep two streams busy at once."""
    f = Front()
    yield f
    f.b.close()


class Probe(object):
    """A probe handle P of one alignment type: created with the poison arena X' (arena 1), with the pinned arenas and the
    pinned destinations of the asynchronous readers."""

    def __init__(self, oracle, name, arenas=(0, 1), case=None, band=SC.BAND, no_common=True, flags=0):
        from biseqt_amd.batch import RESULT_DTYPE, SUMMARY_DTYPE, BatchAligner, PinnedArray
        self.name = name
        self.exp = {a: SC.expected(oracle, a, name, case, band, no_common) for a in arenas}
        self.arena = {a: SC.layout(self.exp[a].pairs)[0] for a in arenas}
        self.offs = SC.layout(self.exp[1].pairs)[1]
        self.b = b = BatchAligner(self.exp[1].pairs, flags=flags, **SC.batch_kw(name, band))
        assert np.array_equal(b.arena, self.arena[1])
        assert all(self.arena[a].shape == b.arena.shape and not np.array_equal(self.arena[a], b.arena) for a in arenas if a != 1)
        self.pin = {a: _pinned(self.arena[a]) for a in arenas}
        self.p_res = PinnedArray(32 * b.n, RESULT_DTYPE)
        self.p_sum = PinnedArray(48 * b.n, SUMMARY_DTYPE)
        self.p_tx = PinnedArray(b.transcripts_bytes)
        self.p_tot = PinnedArray(8, np.uint64)
        self.n_cols = len(b.arena)

    def poison(self, full=True):
        """Every stage on the default stream with X': records, slots, summaries, CIGAR runs, packed bytes and offsets, and the
        pinned destinations, all hold X' answers afterwards."""
        b = self.b
        b.upload_async(self.pin[1])
        b.solve()
        b.traceback()
        b.pack_transcripts()
        b.packed_total_async(self.p_tot)
        b.results_async(self.p_res)
        b.transcripts_async(self.p_tx)
        if full:
            b.summarize()
            b.summaries_async(self.p_sum)
            b.cigars('extended')
        b.sync()
        self.check_records(1, self.p_res.array, self.p_tx.array, 'poison')

    def check_records(self, a, res, slots, what):
        got = SC.view_of(res, self.b.transcripts(res, slots=slots))
        want = self.exp[a].view
        bad = [k for k in range(len(want)) if got[k] != want[k]]
        assert not bad, (self.name, what, 'arena %d' % a, bad[:8], got[bad[0]], want[bad[0]])

    def check_packed(self, a, buf, off, what):
        e = self.exp[a]
        assert np.array_equal(off, e.packed_offsets), (self.name, what, 'packed offsets')
        assert np.array_equal(buf[:int(off[-1])], e.packed_bytes), (self.name, what, 'packed bytes')

    def close(self):
        self.b.close()
        for p in list(self.pin.values()) + [self.p_res, self.p_sum, self.p_tx, self.p_tot]:
            p.close()


def _busy(st, flags, what):
    """Reads ``stream.query()`` right behind a critical call: False while the device still works."""
    flags.append((what, st.query()))


def _assert_busy(flags):
    idle = [w for w, done in flags if done is not False]
    assert not idle, 'the stream was idle behind %s: the front load is too small for this probe' % (idle,)


def _short_chain(p, a, st, flags):
    """upload, solve, traceback, pack and the asynchronous readers of records, slots and the packed total."""
    b, s = p.b, st.cuda_stream
    b.upload_async(p.pin[a], s); _busy(st, flags, 'upload_async')
    b.solve(s); _busy(st, flags, 'solve')
    b.traceback(s); _busy(st, flags, 'traceback')
    b.pack_transcripts(s); _busy(st, flags, 'pack_transcripts')
    b.packed_total_async(p.p_tot, s); _busy(st, flags, 'packed_total_async')
    b.results_async(p.p_res, s); _busy(st, flags, 'results_async')
    b.transcripts_async(p.p_tx, s); _busy(st, flags, 'transcripts_async')


def _check_short(p, a, what):
    b, e = p.b, p.exp[a]
    p.check_records(a, p.p_res.array, p.p_tx.array, what + ', pinned')
    assert int(p.p_tot.array[0]) == len(e.packed_bytes), (what, 'pinned total')
    res = b.results()
    assert np.array_equal(res, p.p_res.array)
    p.check_records(a, res, None, what + ', synchronous readers')
    p.check_packed(a, *b.packed(), what=what)


# ---- 1. the whole chain on one stream ----------------------------------------------------------------------------
HOST_MS = {}


@pytest.mark.parametrize('name', sorted(SC.TYPES))
def test_whole_chain_on_one_stream(oracle, front, name):
    """Every asynchronous stage of a batch behind F on one stream, three times on one handle: Y, the poison again, Y."""
    from biseqt_amd.batch import RESULT_DTYPE, SUMMARY_DTYPE, Pileup
    st, = _streams(1)
    s = st.cuda_stream
    p = Probe(oracle, name)
    b = p.b
    piles = [Pileup(p.n_cols, 4) for _ in range(3)]
    try:
        p.poison()
        for rnd, (a, form) in enumerate(((0, 'extended'), (1, 'classic'), (0, 'classic'))):
            what, e, pile, flags = 'round %d' % rnd, p.exp[a], piles[rnd], []
            front.queue(st)
            t0 = time.perf_counter()
            _short_chain(p, a, st, flags)
            b.summarize(s); _busy(st, flags, 'summarize')
            b.summaries_async(p.p_sum, s); _busy(st, flags, 'summaries_async')
            b.pileup_add(pile, stream=s); _busy(st, flags, 'pileup_add')
            _busy(st, flags, 'in front of cigars')
            HOST_MS[name, rnd] = 1e3 * (time.perf_counter() - t0)
            cig = b.cigars(form, s)                              # (blocks on the stream once, by contract)
            other = 'classic' if form == 'extended' else 'extended'
            st.synchronize()
            print('streams probe: %s %s: chain queued in %.3f ms of host time' % (name, what, HOST_MS[name, rnd]))
            _assert_busy(flags)
            front.check()
            # pinned copies, the synchronous readers and the device views
            _check_short(p, a, what)
            p.check_records(a, _dev(b.results_device(), RESULT_DTYPE), _dev(b.transcripts_device()), what + ', device views')
            tx_summary_ref.assert_equal(p.p_sum.array, e.summaries, what + ', pinned summaries')
            tx_summary_ref.assert_equal(b.summaries(), e.summaries, what + ', summaries()')
            tx_summary_ref.assert_equal(_dev(b.summaries_device(), SUMMARY_DTYPE), e.summaries, what + ', summaries_device')
            d_buf, d_off = b.packed_device()
            p.check_packed(a, _dev(d_buf), _dev(d_off, np.uint64), what + ', packed_device')
            cigar_ref.assert_equal(cig, e.txs, FORMS[form], what + ', cigars on the stream')
            d_runs, d_offs = b.cigars_device()
            cigar_ref.assert_equal((_dev(d_runs, np.uint32), _dev(d_offs, np.uint64)), e.txs, FORMS[form], what + ', cigars_device')
            cigar_ref.assert_equal(b.cigars(other, s), e.txs, FORMS[other], what + ', the other form')
            want = e.pileup(p.n_cols)
            assert want.any()
            got = pile.counts()
            assert (got == want).all(), (name, what, np.argwhere(got != want)[:8])
            assert (_dev(pile.counts_device(), np.uint32).reshape(want.shape) == want).all()
    finally:
        for pile in piles:
            pile.close()
        p.close()


# ---- 2. kernel families --------------------------------------------------------------------------------------------
# (id, type, flags name, kernel substrings / excluded substring, env)
FAMILIES = [
    ('fill16-wave', 'b_local', None, (['k_fill16<'], '_mw'), {}),
    ('fill16-mw', 'b_local', None, (['k_fill16_mw'], None), {'PWLIB_LATENCY_MODE': '1'}),
    ('fill-i32', 'b_local', 'NO_PACKED16', (['k_fill<int'], None), {}),
    ('fill-f64', 'b_local', 'FORCE_F64', (['k_fill<double'], None), {}),
    ('tiled', 'global', 'FORCE_TILED', (['k_fill_tile'], None), {}),
    ('strip', 'global', 'FORCE_STRIP', (['strip'], None), {'PWLIB_NO_STRIP_REPAIR': '1'}),
]


@pytest.mark.parametrize('fam', FAMILIES, ids=[f[0] for f in FAMILIES])
def test_kernel_families_on_a_stream(oracle, front, fam, monkeypatch):
    """Records, transcripts and packed bytes of one probe per fill family, behind F on a stream.  The strip pipeline runs
    alone on its stream with no F in front (its wavefronts wait on each other by design: nothing else may starve them); its
    own fill is the load there."""
    from biseqt_amd import _pwlib as W
    fid, name, flag, (names, excluded), env = fam
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kw = {}
    if fid in SC.FAMILY_CASES:
        name, case, band, no_common = SC.FAMILY_CASES[fid]
        kw = dict(case=case, band=band, no_common=no_common)
    st, = _streams(1)
    p = Probe(oracle, name, flags=getattr(W, 'PW_FLAG_' + flag) if flag else 0, **kw)
    try:
        kname = p.b.kernel_name
        assert all(x in kname for x in names) and not (excluded and excluded in kname), (fid, kname)
        assert all(p.exp[0].view[k] != p.exp[1].view[k] for k in range(p.b.n)), fid
        p.poison(full=False)
        flags = []
        if fid != 'strip':
            front.queue(st)
        _short_chain(p, 0, st, flags)
        st.synchronize()
        if fid == 'strip':
            # With no F in front the only load is the pair's own fill and walk, which nothing sizes against the host's
            # queueing time: the stream must be busy behind solve (the fill has just been launched); the flags behind the
            # later calls are printed, not asserted.
            print('streams probe: strip: stream done behind %s' % (flags,))
            flags = [f for f in flags if f[0] == 'solve']
        _assert_busy(flags)
        if fid != 'strip':
            front.check()
        _check_short(p, 0, fid + ' on ' + kname)
    finally:
        p.close()


# ---- 3. two batches in flight ----------------------------------------------------------------------------------------
def test_two_batches_in_flight(oracle, front, front2):
    """bench.py's loop in small: handles A and B on streams 0 and 1, six steps, step i on handle i % 2 with arena i % 3; a
    handle is queued again only after the step two back was synchronised and checked.  Each stream has its own front load
    in front of every step."""
    sts = _streams(2)
    fronts = (front, front2)
    ps = [Probe(oracle, 'b_local', arenas=(0, 1, 2)) for _ in range(2)]
    try:
        for p in ps:
            p.poison(full=False)

        def check(i):
            h, a = i % 2, i % 3
            sts[h].synchronize()
            p, e = ps[h], ps[h].exp[a]
            what = 'step %d' % i
            p.check_records(a, p.p_res.array, None, what + ', pinned records')          # (slots: the synchronous reader)
            assert int(p.p_tot.array[0]) == len(e.packed_bytes), (what, 'pinned total')
            p.check_packed(a, *p.b.packed(), what=what)
            fronts[h].check()

        flags = []
        for i in range(6):
            h, a = i % 2, i % 3
            if i >= 2:
                check(i - 2)
            b, st = ps[h].b, sts[h]
            s = st.cuda_stream
            fronts[h].queue(st)
            b.upload_async(ps[h].pin[a], s); _busy(st, flags, 'upload_async %d' % i)
            b.solve(s); _busy(st, flags, 'solve %d' % i)
            b.traceback(s); _busy(st, flags, 'traceback %d' % i)
            b.pack_transcripts(s); _busy(st, flags, 'pack_transcripts %d' % i)
            b.results_async(ps[h].p_res, s); _busy(st, flags, 'results_async %d' % i)
            b.packed_total_async(ps[h].p_tot, s); _busy(st, flags, 'packed_total_async %d' % i)
        check(4)
        check(5)
        _assert_busy(flags)
    finally:
        for p in ps:
            p.close()


# ---- 4. cross-stream calls on one handle -------------------------------------------------------------------------------
def test_cross_stream_calls_on_one_handle(oracle, front, front2):
    """The second call of each kind comes on another stream while the first is still queued behind F.  The caller orders only
    the PRODUCERS: one event recorded on s0 right behind the traceback, which s1 waits for.  Nothing of the caller's orders
    the consumers of the two streams against each other: the library's own buffers (CIGAR offsets and runs, the col0
    staging, summaries, packed bytes) are the library's business.

    What this shows and what it cannot.  Summaries and packed bytes are written twice with the same content, so they must
    come out right whatever the order.  The guards of the CIGAR buffers and of the col0 staging protect a window between two
    adjacent commands of ONE stream (the staged copy and the kernel that reads it; the count, its blocking read and the write
    kernel): no front load can hold that window open, so without the guards the results would be wrong only now and then.
    What a guard does every time is wait on the host for the other stream; for col0 that is read here (s0 has drained when
    the call on s1 returns -- a guard that ordered the streams on the device instead would be as good, and this line would
    then go)."""
    import torch
    from biseqt_amd.batch import Pileup
    s0, s1 = _streams(2)
    p = Probe(oracle, 'global')
    b, e = p.b, p.exp[0]
    origin_off = np.array([oo for oo, _ in p.offs], np.int64)
    col_a, col_b = origin_off + 16, origin_off.copy()
    col_b[::3] = -1                                                    # (every third pair skipped)
    piles = [Pileup(p.n_cols + 16, 4) for _ in range(2)]
    try:
        p.poison()
        flags = []
        front.queue(s0)
        _short_chain(p, 0, s0, flags)
        ev = torch.cuda.Event(); ev.record(s0); s1.wait_event(ev)       # the producers, and nothing behind them
        # summaries and packed transcripts, queued twice: each stream behind a front load of its own
        front.queue(s0)
        front2.queue(s1)
        b.summarize(s0.cuda_stream); _busy(s0, flags, 'summarize on s0')
        b.pack_transcripts(s0.cuda_stream); _busy(s0, flags, 'pack_transcripts on s0')
        b.summarize(s1.cuda_stream); _busy(s1, flags, 'summarize on s1')
        b.pack_transcripts(s1.cuda_stream); _busy(s1, flags, 'pack_transcripts on s1')
        b.summaries_async(p.p_sum, s1.cuda_stream); _busy(s1, flags, 'summaries_async on s1')
        # CIGARs: extended on s0, entered while s0 is busy (the call blocks once and returns with its write kernel queued),
        # classic on s1 at once
        _busy(s0, flags, 'in front of cigars extended')
        assert b.lib.pw_batch_cigars(b.handle, FORMS['extended'], s0.cuda_stream) == 0
        cla = b.cigars('classic', s1.cuda_stream)
        cigar_ref.assert_equal(cla, e.txs, FORMS['classic'], 'classic on s1 behind extended on s0')
        ext = b.cigars('extended', s0.cuda_stream)
        cigar_ref.assert_equal(ext, e.txs, FORMS['extended'], 'extended on s0 behind classic on s1')
        # pileups: two col0 arrays through the one staging buffer; the add on s0 is still queued behind F when the call on
        # s1 comes (that call waits on the host, so nothing is read behind it but s0 itself)
        front.queue(s0)
        b.pileup_add(piles[0], col0=col_a, stream=s0.cuda_stream); _busy(s0, flags, 'pileup_add on s0')
        b.pileup_add(piles[1], col0=col_b, stream=s1.cuda_stream)
        drained = s0.query()
        s0.synchronize()
        s1.synchronize()
        _assert_busy(flags)
        assert drained is True, 'pw_batch_pileup_add on s1 did not wait for the add still queued on s0'
        front.check()
        front2.check()
        for pile, col in zip(piles, (col_a, col_b)):
            want = e.pileup(p.n_cols + 16, col)
            got = pile.counts()
            assert want.any() and (got == want).all(), np.argwhere(got != want)[:8]
        assert (piles[0].counts() != piles[1].counts()).any()
        tx_summary_ref.assert_equal(p.p_sum.array, e.summaries, 'summaries on s1 beside s0')
        tx_summary_ref.assert_equal(b.summaries(), e.summaries, 'summaries()')
        p.check_packed(0, *b.packed(), what='packed on s1 beside s0')
        _check_short(p, 0, 'cross-stream')
    finally:
        for pile in piles:
            pile.close()
        p.close()


# ---- 5. host arrays are consumed at return -----------------------------------------------------------------------------
@pytest.mark.parametrize('memory', ['pageable', 'pinned'])
@pytest.mark.parametrize('name', ['global', 'b_local'])
def test_host_arrays_are_consumed_at_return(oracle, front, name, memory):
    """``ends_ij`` of pw_batch_traceback_from and ``col0`` of pw_batch_pileup_add are arrays of the caller -- pageable numpy
    arrays that Python frees when the wrapper returns, or page-locked ones of a ring that is refilled for the next step:
    overwritten right behind the call, while the stream is still busy with F, what they held at the call must reach the
    device."""
    from biseqt_amd.batch import Pileup
    st, = _streams(1)
    s = st.cuda_stream
    p = Probe(oracle, name)
    b, e = p.b, p.exp[0]
    pile, held = Pileup(p.n_cols + 16, 4), []
    try:
        p.poison(full=False)
        want_col0 = np.array([oo + 16 for oo, _ in p.offs], np.int64)
        if memory == 'pinned':
            held = [_pinned(e.ends.reshape(-1), np.int32), _pinned(want_col0, np.int64)]
            ends, col0 = held[0].array, held[1].array
        else:
            ends, col0 = e.ends.reshape(-1).copy(), want_col0.copy()    # every pair's optimal cell, (-1, -1) without one
        flags = []
        front.queue(st)
        b.upload_async(p.pin[0], s)
        b.solve(s); _busy(st, flags, 'solve')
        assert b.lib.pw_batch_traceback_from(b.handle, ends.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), s) == 0
        _busy(st, flags, 'traceback_from')
        ends[:] = -1
        assert b.lib.pw_batch_pileup_add(b.handle, pile.handle, col0.ctypes.data, 0, s) == 0
        _busy(st, flags, 'pileup_add')
        col0[:] = -1
        b.results_async(p.p_res, s)
        b.transcripts_async(p.p_tx, s)
        st.synchronize()
        _assert_busy(flags)
        front.check()
        res = p.p_res.array
        txs = b.transcripts(res, slots=p.p_tx.array)
        assert sum(1 for t in txs if t) >= 48
        okw = SC.oracle_kw(name)
        for k, (o, m) in enumerate(e.pairs):                             # the oracle's traceback_from at the original cells
            check_walks(oracle, o, m, okw, [tuple(e.ends[k])], res[k:k + 1], txs[k:k + 1], '%s pair %d' % (name, k))
        # ... which are the optimal cells: the transcripts of Y, where the poison run left those of X'
        assert [t for t, w in zip(txs, e.txs) if w] == [w for w in e.txs if w]
        want = e.pileup(p.n_cols + 16, want_col0)
        got = pile.counts()
        assert want.any() and (got == want).all(), np.argwhere(got != want)[:8]
    finally:
        for h in held:
            h.close()
        pile.close()
        p.close()


# ---- 6. destroy in flight, then reuse from the pool --------------------------------------------------------------------
def test_destroy_in_flight_then_reuse_from_the_pool(front):
    """A batch is closed with its work still queued behind F; the next batch of the same shape takes its parked buffers
    (not zeroed) at once and runs on another stream.  Both record sets equal default-stream runs on fresh handles."""
    from biseqt_amd import synth, _pwlib as W
    from biseqt_amd.batch import RESULT_DTYPE, BatchAligner, PinnedArray
    lib = W.load()
    kw = dict(alnmode=1, alntype=1, alphabet_len=4, diag_range=(-150, 150), **SC.SCORES)
    sets = [list(zip(*synth.pair_batch(seed, 1000, 600))) for seed in (5301, 5302)]

    def used():
        free, total = ctypes.c_uint64(), ctypes.c_uint64()
        assert lib.pw_device_memory(0, ctypes.byref(free), ctypes.byref(total)) == 0
        return (total.value - free.value) / 2.0 ** 20

    refs = []
    for pairs in sets:
        with BatchAligner(pairs, **kw) as b:
            refs.append(b.run().copy())
    assert not np.array_equal(refs[0]['score'], refs[1]['score'])
    s0, s1 = _streams(2)
    pins = [PinnedArray(32 * 1000, RESULT_DTYPE) for _ in range(2)]
    lib.pw_pool_trim()
    base = used()
    flags = []
    b1 = b2 = arena1 = None
    try:
        b1 = BatchAligner(sets[0], upload=False, **kw)
        arena1 = _pinned(b1.arena)
        held = used() - base
        assert held > 8, held                                      # MB: large enough for the pool to park
        front.queue(s0)
        b1.upload_async(arena1, s0.cuda_stream)
        b1.solve(s0.cuda_stream)
        b1.traceback(s0.cuda_stream)
        b1.results_async(pins[0], s0.cuda_stream); _busy(s0, flags, 'in front of close')
        b1.close()                                                 # no sync by the caller: ~pw_batch waits for its events
        parked = used() - base
        b2 = BatchAligner(sets[1], **kw)
        after = used() - base
        b2.solve(s1.cuda_stream)
        b2.traceback(s1.cuda_stream)
        b2.results_async(pins[1], s1.cuda_stream)
        s1.synchronize()
        s0.synchronize()
        _assert_busy(flags)
        assert np.array_equal(pins[0].array, refs[0])
        assert np.array_equal(pins[1].array, refs[1])
        assert np.array_equal(b2.results(), refs[1])
        front.check()
        # the second batch took parked buffers: the memory in use did not grow by another batch
        assert parked > held / 2, (held, parked)
        assert after - parked < held / 4, (held, parked, after)
    finally:
        s0.synchronize()
        s1.synchronize()
        for h in (b1, b2, arena1) + tuple(pins):
            if h is not None:
                h.close()
        lib.pw_pool_trim()
    assert used() - base < 32


# ---- 7. one pileup, two streams ----------------------------------------------------------------------------------------
def test_one_pileup_two_streams(oracle, front, front2):
    """Two handles on two streams add into one pileup concurrently (atomic adds on shared columns); the call runs on s0
    behind an event wait on s1.  ``clear`` queued between two adds on one stream leaves exactly the second add."""
    import torch
    from biseqt_amd.batch import DeviceArena, Pileup
    s0, s1 = _streams(2)
    pa, pb = Probe(oracle, 'global', arenas=(0, 1)), Probe(oracle, 'global', arenas=(2, 1))
    n_cols = pa.n_cols + 16
    shifted = np.array([oo + 16 for oo, _ in pa.offs], np.int64)
    pile, pile2 = Pileup(n_cols, 4), Pileup(n_cols, 4)
    ref = np.concatenate([pa.arena[0], np.zeros(16, np.uint8)])
    ref_dev = DeviceArena(ref)
    try:
        pa.poison(full=False)
        pb.poison(full=False)
        flags = []
        front.queue(s0)
        front2.queue(s1)
        for p, a, st in ((pa, 0, s0), (pb, 2, s1)):
            s = st.cuda_stream
            p.b.upload_async(p.pin[a], s)
            p.b.solve(s)
            p.b.traceback(s)
            p.b.pileup_add(pile, stream=s); _busy(st, flags, 'pileup_add of arena %d' % a)
        ev = torch.cuda.Event(); ev.record(s1); s0.wait_event(ev)
        pile.call((ref_dev, 0), min_depth=2, stream=s0.cuda_stream); _busy(s0, flags, 'call')
        # clear between two adds on one stream
        pa.b.pileup_add(pile2, col0=shifted, stream=s0.cuda_stream)
        pile2.clear(s0.cuda_stream)
        pa.b.pileup_add(pile2, stream=s0.cuda_stream); _busy(s0, flags, 'add, clear, add')
        s0.synchronize()
        s1.synchronize()
        _assert_busy(flags)
        front.check()
        front2.check()
        want = pa.exp[0].pileup(n_cols) + pb.exp[2].pileup(n_cols)
        assert want.max() >= 2
        got = pile.counts()
        assert (got == want).all(), np.argwhere(got != want)[:8]
        sites = pileup_ref.call(want, 4, ref, 2)
        assert np.array_equal(pile.sites(), sites)
        assert (sites['flags'] & pileup_ref.DIFFERS).any() and (sites['flags'] & pileup_ref.COVERED).any()
        assert (pile2.counts() == pa.exp[0].pileup(n_cols)).all()
        assert (pa.exp[0].pileup(n_cols, shifted) != pa.exp[0].pileup(n_cols)).any()
    finally:
        pile.close()
        pile2.close()
        ref_dev.close()
        pa.close()
        pb.close()


# ---- 8. builds on a stream ---------------------------------------------------------------------------------------------
class _Kmers(object):
    """The C calls of include/pw_kmers.h on one handle, the build on a stream."""

    def __init__(self, L, k):
        from biseqt_amd import _pwlib as W
        self.lib = W.load()
        self.h = self.lib.pw_kmers_create(0, L, k)
        assert self.h

    def build(self, reads, strands, comp, stream):
        lens = np.array([len(r) for r in reads], np.int32)
        offs = np.zeros(len(reads) + 1, np.uint64)
        offs[1:] = np.cumsum(lens, dtype=np.uint64)
        arena = np.ascontiguousarray(np.concatenate([np.asarray(r, np.uint8) for r in reads]))
        roff = np.ascontiguousarray(offs[:-1])
        comp = np.ascontiguousarray(comp, np.uint8)
        rc = self.lib.pw_kmers_build(self.h, arena.ctypes.data, arena.size, roff.ctypes.data, lens.ctypes.data, len(reads),
                                     3 if strands == 'both' else 1, comp.ctypes.data, stream)
        assert rc == 0, (self.lib.pw_kmers_last_error() or b'').decode()

    def check(self, reads, k, L, strands, comp):
        lib, h = self.lib, self.h
        u, c = KR.counts(reads, k, L, strands, comp)
        n = lib.pw_kmers_num_distinct(h)
        assert n == len(u) and lib.pw_kmers_num_entries(h) == len(KR.table(reads, k, L, strands, comp)[0])
        keys, cnt = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
        assert lib.pw_kmers_distinct(h, keys.ctypes.data, cnt.ctypes.data, n) == 0
        assert np.array_equal(keys, u) and np.array_equal(cnt, c)
        q = np.array(u[::-1].tolist() + [L ** k, 2 ** 64 - 1] + u[:2].tolist(), np.uint64)
        out = np.full(len(q), 0xdeadbeef, np.uint32)
        assert lib.pw_kmers_lookup(h, q.ctypes.data, len(q), out.ctypes.data) == 0
        assert np.array_equal(out, KR.lookup(reads, k, L, q, strands, comp))
        top = int(c.max())
        hist = np.full(top + 1, 0xdeadbeef, np.uint64)
        assert lib.pw_kmers_spectrum(h, top, hist.ctypes.data) == 0
        assert np.array_equal(hist, KR.spectrum(c, top))
        want = KR.occurrences(reads, k, L, strands, comp)
        occ = np.full(len(want), 0xdeadbeef, np.uint32)
        assert lib.pw_kmers_occurrences(h, occ.ctypes.data) == 0
        assert np.array_equal(occ, want)

    def close(self):
        self.lib.pw_kmers_destroy(self.h)


@pytest.mark.parametrize('strands', ['+', 'both'])
def test_kmer_build_on_a_stream(front, strands):
    """pw_kmers_build behind F on a stream, then every query; then two builds of one handle on two streams back to back
    (the second waits for the first: nobody has asked for its number of runs yet)."""
    s0, s1 = _streams(2)
    k, L, comp = KR.PLANTED_K, KR.PLANTED_L, KR.DNA_COMPLEMENT
    t = _Kmers(L, k)
    try:
        flags = []
        front.queue(s0)
        _busy(s0, flags, 'in front of the build')
        t.build(KR.planted_reads(0), strands, comp, s0.cuda_stream)
        _assert_busy(flags)
        t.check(KR.planted_reads(0), k, L, strands, comp)
        t.build(KR.planted_reads(2), strands, comp, s0.cuda_stream)
        t.build(KR.planted_reads(1), strands, comp, s1.cuda_stream)
        t.check(KR.planted_reads(1), k, L, strands, comp)
        s0.synchronize()
        front.check()
    finally:
        t.close()


def test_seed_index_builds_on_a_stream(front):
    """The three seed-index builds with a stream argument, entered while the stream is busy with F: rows equal the oracles."""
    from biseqt_amd.seeds import _Index, _MIndex, _QIndex
    from biseqt_amd.sequence import Alphabet
    from oracle import seeds_oracle as SO
    from tests import mseeds_cases as MC, overlap_cases as OC, qseeds_cases as QC
    A = Alphabet('ACGT')
    st, = _streams(1)
    s = st.cuda_stream
    c = [x for x in OC.cases() if x.name == 'table_513'][0]
    S, T = c.reads
    mc = MC.every_n(3)
    qc = QC.many_queries_in_one_workgroup()
    assert c.alphabet_len == 4 and mc['L'] == 4 and qc['L'] == 4
    pair, multi = _Index(S, T, c.wordlen, A, self_comp=0), _MIndex(mc['seqs'], mc['wordlen'], A)
    many = _QIndex(qc['ref'], qc['wordlen'], A)
    try:
        flags = []
        front.queue(st)
        _busy(st, flags, 'in front of pw_seeds_build')
        pair.build(stream=s)
        front.queue(st)
        _busy(st, flags, 'in front of pw_mseeds_build')
        multi.build(stream=s)
        front.queue(st)
        _busy(st, flags, 'in front of pw_qseeds_build')
        many.build(*QC.pack_tight(qc['queries']), stream=s)
        st.synchronize()
        _assert_busy(flags)
        front.check()
        rows, _ = SO.seed_rows(S, T, c.wordlen, 4, [])
        assert len(rows) > 0 and [tuple(r) for r in pair.rows().tolist()] == rows
        want = MC.rows_of(mc)
        assert len(want) > 0 and np.array_equal(multi.rows(), want)
        want, off = QC.rows_of(qc)
        assert len(want) > 0 and np.array_equal(many.rows(), want) and np.array_equal(many.row_offsets(), off)
    finally:
        pair.close()
        multi.close()
        many.close()
