"""The batch API's refusals after pw_batch_create: each is reported with its full message (pw_last_error), leaves the batch
usable, and the next correct call on the same batch succeeds and computes what a fresh batch computes."""
import ctypes as C

import numpy as np
import pytest

from biseqt_amd import synth

pytestmark = pytest.mark.gpu

_KW = dict(alnmode=0, alntype=1, alphabet_len=4, match_score=1, mismatch_score=-3, go_score=-5, ge_score=-2)


def _pairs():
    origins, mutants = synth.pair_batch(11, 6, 300)
    return list(zip(origins, mutants))


def _refused(lib, call, msg):
    """call() returns -1 and leaves exactly `msg` in pw_last_error (which held another message before)."""
    lib.pw_plan_only(None, 0, None, 0, 0, None, 0, None)
    assert lib.pw_last_error() != msg
    assert call() == -1, msg
    assert lib.pw_last_error() == msg, (msg, lib.pw_last_error())


def _dbl(n):
    out = np.zeros(max(n, 1), np.float64)
    return out, out.ctypes.data_as(C.POINTER(C.c_double))


def _expected(pairs, **kw):
    from biseqt_amd.batch import BatchAligner
    with BatchAligner(pairs, **dict(_KW, **kw)) as b:
        res = b.run()
        return res.copy(), b.transcripts(res)


def _same(res, want):
    assert np.array_equal(res['score'], want['score']) and np.array_equal(res['opt_i'], want['opt_i']) and \
        np.array_equal(res['opt_j'], want['opt_j'])


def test_shared_arena_refusals():
    """Solve before pw_batch_share_arena, share_arena without the flag and with NULL, uploads (sync and async) into a batch
    that owns no arena."""
    from biseqt_amd import _pwlib as W
    from biseqt_amd.batch import BatchAligner, DeviceArena
    pairs = _pairs()
    want, _ = _expected(pairs)
    b = BatchAligner(pairs, upload=False, flags=W.PW_FLAG_SHARED_ARENA, **_KW)
    with DeviceArena(b.arena) as dev, b:            # (the batch goes first)
        lib, h = b.lib, b.handle
        _refused(lib, lambda: lib.pw_batch_solve(h, None),
                 b'pw_batch_solve: the batch was created with PW_FLAG_SHARED_ARENA and has no arena yet')
        _refused(lib, lambda: lib.pw_batch_share_arena(h, None), b'pw_batch_share_arena: null arena')
        assert lib.pw_batch_share_arena(h, dev.ptr) == 0
        msg = b'the batch shares a caller-owned arena (PW_FLAG_SHARED_ARENA): nothing to upload'
        _refused(lib, lambda: lib.pw_batch_upload_arena(h, b.arena.ctypes.data, b.arena.nbytes), msg)
        _refused(lib, lambda: lib.pw_batch_upload_arena_async(h, b.arena.ctypes.data, b.arena.nbytes, None), msg)
        _same(b.run(), want)
    b = BatchAligner(pairs, **_KW)
    with DeviceArena(b.arena) as dev, b:
        _refused(b.lib, lambda: b.lib.pw_batch_share_arena(b.handle, dev.ptr),
                 b'pw_batch_share_arena: the batch was not created with PW_FLAG_SHARED_ARENA')
        _same(b.run(), want)


def test_upload_larger_than_the_arena_is_refused():
    from biseqt_amd.batch import BatchAligner, PinnedArray
    pairs = _pairs()
    want, _ = _expected(pairs)
    with BatchAligner(pairs, upload=False, **_KW) as b:
        lib, h = b.lib, b.handle
        big = np.zeros(b.arena.nbytes + 1, np.uint8)
        _refused(lib, lambda: lib.pw_batch_upload_arena(h, big.ctypes.data, big.nbytes), b'arena upload larger than the arena')
        _refused(lib, lambda: lib.pw_batch_upload_arena_async(h, big.ctypes.data, big.nbytes, None),
                 b'arena upload larger than the arena')
        pin = PinnedArray(b.arena.nbytes)
        pin.array[:] = b.arena
        b.upload_async(pin)
        _same(b.run(), want)
        pin.close()


def test_packed_transcript_refusals():
    """pw_batch_packed / pw_batch_packed_total_async before pw_batch_pack_transcripts, pw_batch_packed into a buffer one
    byte too small."""
    from biseqt_amd.batch import BatchAligner, PinnedArray
    pairs = _pairs()
    want, want_tx = _expected(pairs)
    with BatchAligner(pairs, **_KW) as b:
        lib, h = b.lib, b.handle
        _same(b.run(), want)
        off = np.zeros(b.n + 1, np.uint64)
        _refused(lib, lambda: lib.pw_batch_packed(h, None, 0, off.ctypes.data), b'pw_batch_packed before pw_batch_pack_transcripts')
        _refused(lib, lambda: lib.pw_batch_packed_total_async(h, off.ctypes.data, None),
                 b'pw_batch_packed_total_async before pw_batch_pack_transcripts')
        b.pack_transcripts()
        total = PinnedArray(8, np.uint64)
        b.packed_total_async(total)
        b.sync()
        assert lib.pw_batch_packed(h, None, 0, off.ctypes.data) == 0 and int(off[-1]) == int(total.array[0]) > 0
        buf = np.zeros(int(off[-1]), np.uint8)
        _refused(lib, lambda: lib.pw_batch_packed(h, buf.ctypes.data, buf.nbytes - 1, None), b'packed transcripts: buffer too small')
        assert lib.pw_batch_packed(h, buf.ctypes.data, buf.nbytes, None) == 0
        assert b.transcripts_from_packed(buf, off) == want_tx
        total.close()


def test_score_plane_and_mask_refusals():
    """pw_batch_scores / pw_batch_table without PW_FLAG_DUMP_SCORES, with k out of range and into a buffer one element too
    small; pw_batch_table on a banded batch; pw_batch_masks out of range and into a buffer one byte too small."""
    from biseqt_amd import _pwlib as W
    from biseqt_amd.batch import BatchAligner
    pairs = _pairs()
    want, _ = _expected(pairs)
    X, Y = len(pairs[0][0]), len(pairs[0][1])
    with BatchAligner(pairs, **_KW) as b:
        lib, h = b.lib, b.handle
        _same(b.run(), want)
        out, p = _dbl((X + 1) * (Y + 1))
        _refused(lib, lambda: lib.pw_batch_scores(h, 0, p, out.size), b'no score plane')
        _refused(lib, lambda: lib.pw_batch_table(h, 0, p, out.size), b'no score plane')
        cells = int(lib.pw_batch_pair_cells(h, 0))
        masks = np.zeros(cells, np.uint8)
        mp = masks.ctypes.data_as(C.POINTER(C.c_uint8))
        for k in (-1, b.n):
            _refused(lib, lambda: lib.pw_batch_masks(h, k, mp, cells), b'no mask plane for this pair')
        _refused(lib, lambda: lib.pw_batch_masks(h, 0, mp, cells - 1), b'mask buffer too small')
        assert lib.pw_batch_masks(h, 0, mp, cells) == 0 and masks.any()
    with BatchAligner(pairs, flags=W.PW_FLAG_DUMP_SCORES, **_KW) as b:
        lib, h = b.lib, b.handle
        _same(b.run(), want)
        dmin, dmax, _ = b.band(0)
        nd, pitch = dmax - dmin + 1, min(X, Y) + 1
        for k in (-1, b.n):
            _refused(lib, lambda: lib.pw_batch_scores(h, k, p, out.size), b'no score plane')
            _refused(lib, lambda: lib.pw_batch_table(h, k, p, out.size), b'no score plane')
        plane, pp = _dbl(nd * pitch)
        _refused(lib, lambda: lib.pw_batch_scores(h, 0, pp, plane.size - 1), b'score buffer too small')
        assert lib.pw_batch_scores(h, 0, pp, plane.size) == 0
        _refused(lib, lambda: lib.pw_batch_table(h, 0, p, out.size - 1), b'table buffer too small')
        assert lib.pw_batch_table(h, 0, p, out.size) == 0
        assert out.max() == want['score'][0]
    banded = dict(_KW, alnmode=1, diag_range=(-40, 40))
    with BatchAligner(pairs, flags=W.PW_FLAG_DUMP_SCORES, **banded) as b:
        lib, h = b.lib, b.handle
        bwant, _ = _expected(pairs, alnmode=1, diag_range=(-40, 40))
        _same(b.run(), bwant)
        _refused(lib, lambda: lib.pw_batch_table(h, 0, p, out.size), b'pw_batch_table: standard mode only')
        _same(b.run(), bwant)
        assert b.scores_plane(0).shape == (81, min(X, Y) + 1)
