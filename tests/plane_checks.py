"""Comparisons of a GPU batch with the oracle that several GPU test files share: the oracle's and the batch's keywords of one
problem, whole tie-mask planes (``check_masks``) and walks from explicit end cells (``check_walks``).  Used by
tests/test_gpu_whole_plane.py and tests/test_gpu_strip_edges.py."""
import numpy as np


def okw_of(kw):
    out = dict(mode=kw['mode'], alntype=kw['alntype'], L=4, go=kw['go'], ge=kw['ge'])
    if 'subst' in kw:
        out['subst'] = kw['subst']
    else:
        out.update(match=kw['match'], mismatch=kw['mismatch'])
    if 'diag_range' in kw:
        out['diag_range'] = kw['diag_range']
    return out


def bkw_of(kw):
    out = dict(alnmode=kw['mode'], alntype=kw['alntype'], alphabet_len=4, go_score=kw['go'], ge_score=kw['ge'])
    if 'subst' in kw:
        out['subst_scores'] = kw['subst']
    else:
        out.update(match_score=kw['match'], mismatch_score=kw['mismatch'])
    if 'diag_range' in kw:
        out['diag_range'] = kw['diag_range']
    return out


def check_masks(oracle, b, k, o, m, okw, no_m, label):
    want = oracle.solve(o, m, want_table=True, **okw)
    got = b.masks(k)
    bits = 7 if no_m else 15
    if no_m:
        assert okw['go'] <= 0, label
    assert got.shape == want['mask'].shape, label
    bad = np.nonzero((got & bits) != (want['mask'] & bits))[0]
    assert bad.size == 0, (label, k, '%d of %d cells differ' % (bad.size, got.size), bad[:8].tolist())
    return want


def check_walks(oracle, o, m, okw, ends, res, txs, label):
    for k, e in enumerate(ends):
        if e[0] < 0:
            assert res['tx_len'][k] == 0 and res['status'][k] == 0, (label, k)
            continue
        r = oracle.traceback_from(o, m, e, **okw)
        if r['no_choice']:
            continue
        st = int(res['status'][k])
        assert st & 1 and not st & 8, (label, e, st)
        g = (txs[k] or '', (int(res['origin_idx'][k]), int(res['mutant_idx'][k])), bool(st & 4),
             bool(st & 2) and not st & 4)
        assert g[1:] == (r['start'], r['would_panick'], r['tb_null']), (label, e, g, r)
        if not st & 2:
            assert g[0] == r['ops'], (label, e)
