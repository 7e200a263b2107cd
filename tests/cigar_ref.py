"""The oracle of the CIGARs (include/pw_cigar.h) in pure Python: ``itertools.groupby`` over the transcript string, the
host work the device runs replace."""
import itertools

import numpy as np

EXTENDED, CLASSIC = 0, 1
OPS = {EXTENDED: {'M': 7, 'S': 8, 'I': 1, 'D': 2}, CLASSIC: {'M': 0, 'S': 0, 'I': 1, 'D': 2}}
LETTERS = 'MIDNSHP=X'                                   # BAM's op letters by code
ST_TRACED, ST_EMPTY, ST_PANICK, ST_BADPATH = 1, 2, 4, 8
FORMS = (('extended', EXTENDED), ('classic', CLASSIC))
EXHAUSTIVE = [''.join(t) for n in range(7) for t in itertools.product('MSID', repeat=n)]
assert len(EXHAUSTIVE) == 5461


def runs(tx, form, status=ST_TRACED):
    """The run dwords ``(length << 4) | op`` of transcript ``tx`` (a ``str`` or None) of a pair with the ``PW_ST_*`` bits
    ``status``: none without a transcript, for an empty one, or for a record the header excludes."""
    if not tx or not status & ST_TRACED or status & (ST_EMPTY | ST_PANICK | ST_BADPATH):
        return []
    return [(len(list(g)) << 4) | op for op, g in itertools.groupby(OPS[form][c] for c in tx)]


def string(tx, form, status=ST_TRACED):
    return ''.join('%d%s' % (r >> 4, LETTERS[r & 15]) for r in runs(tx, form, status))


def packed(txs, form, statuses=None):
    """``(runs uint32[total], offsets uint64[n + 1])`` of a list of transcripts."""
    per = [runs(t, form, ST_TRACED if statuses is None else int(statuses[k])) for k, t in enumerate(txs)]
    off = np.zeros(len(per) + 1, np.uint64)
    if per:
        off[1:] = np.cumsum([len(p) for p in per])
    return np.array([r for p in per for r in p], np.uint32), off


def assert_equal(got, txs, form, what='', statuses=None):
    """``got = (runs, offsets)`` equals the oracle on ``txs``, pair by pair."""
    g_runs, g_off = got
    e_runs, e_off = packed(txs, form, statuses)
    assert g_off.dtype == np.uint64 and g_runs.dtype == np.uint32, (what, g_off.dtype, g_runs.dtype)
    assert len(g_off) == len(e_off), (what, len(g_off), len(e_off))
    assert int(g_off[-1]) == len(g_runs), (what, int(g_off[-1]), len(g_runs))
    if (g_off == e_off).all() and (g_runs == e_runs).all():
        return
    for k in range(len(txs)):
        g = g_runs[int(g_off[k]):int(g_off[k + 1])].tolist()
        e = e_runs[int(e_off[k]):int(e_off[k + 1])].tolist()
        assert g == e, (what, k, (txs[k] or '')[:80], [(r >> 4, r & 15) for r in g[:12]], [(r >> 4, r & 15) for r in e[:12]])
    raise AssertionError((what, 'offsets differ'))
