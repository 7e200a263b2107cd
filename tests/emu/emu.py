"""ctypes wrapper of the CPU lane emulator (tests/emu/emu_wave.cpp) -- TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, 'libemu_wave.so')
SRC = os.path.join(HERE, 'emu_wave.cpp')
CSRC = os.path.join(os.path.dirname(os.path.dirname(HERE)), 'biseqt_amd', 'csrc')

_lib = None


def build(force=False):
    deps = [SRC] + [os.path.join(CSRC, f) for f in ('pw_wave.h', 'pw_strip.h', 'pw_plan.h', 'pw_model.h', 'pw_types.h')]
    if force or not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(['g++', '-O1', '-std=c++17', '-shared', '-fPIC', '-ffp-contract=off',
                               SRC, '-o', SO])


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(SO)
        _lib.emu_solve.restype = C.c_int
        _lib.emu_solve_strip.restype = C.c_int
    return _lib


def _table_cells(mode, X, Y, dr):
    """Cells of the reference's table (banded: the clamped band's diagonals back to back)."""
    if mode == 0:
        return (X + 1) * (Y + 1)
    dmin, dmax = max(dr[0], -Y), min(dr[1], X)
    return sum(1 + min(d, 0) + min(X - d, Y) for d in range(dmin, dmax + 1))


class _PlaneOut(object):
    """Buffers of the whole-plane read-back (emu_set_masks_out) and of the walks from given end cells (emu_set_ends)."""

    def __init__(self, cells, want_masks, ends, X, Y):
        self.mask = np.zeros(max(cells, 1), np.uint8) if want_masks else None
        self.ends = None if ends is None else np.ascontiguousarray(np.asarray(ends, np.int32).reshape(-1, 2))
        n = 0 if self.ends is None else len(self.ends)
        self.info = np.zeros(4 * max(n, 1), np.int32)
        self.stride = X + Y + 2
        self.tx = C.create_string_buffer(max(n, 1) * self.stride)

    def __enter__(self):
        lib().emu_set_masks_out(None if self.mask is None else self.mask.ctypes.data_as(C.POINTER(C.c_uint8)))
        if self.ends is not None:
            lib().emu_set_ends(self.ends.ctypes.data_as(C.POINTER(C.c_int)), len(self.ends),
                               self.info.ctypes.data_as(C.POINTER(C.c_int)), self.tx, self.stride)
        return self

    def __exit__(self, *a):
        lib().emu_set_masks_out(None)
        lib().emu_set_ends(None, 0, None, None, 0)

    def fill(self, out, cells, orange, mrange):
        """Adds ``mask`` (cells of the table) and ``walks`` (one dict per end cell: origin_idx, mutant_idx, transcript,
        status -- PW_ST_* bits) to a result dict."""
        if self.mask is not None:
            out['mask'] = self.mask[:cells].copy()
        if self.ends is not None:
            raw = self.tx.raw
            walks = []
            for e in range(len(self.ends)):
                o, m, n, st = (int(v) for v in self.info[4 * e:4 * e + 4])
                t = raw[e * self.stride:e * self.stride + n].decode('ascii') if n > 0 else ''
                walks.append(dict(origin_idx=o + orange[0], mutant_idx=m + mrange[0], transcript=t, status=st))
            out['walks'] = walks


def solve(origin, mutant, mode=0, alntype=0, subst=None, L=None, match=1., mismatch=0., go=0., ge=0.,
          diag_range=None, origin_range=None, mutant_range=None, use_double=False, force_generic=False,
          bk=8, want_table=False, packed16=False, waves=1, matrix=None, product_variant=False, want_masks=False, end=None,
          ends=None, **_):
    """One problem on one emulated kernel.  ``packed16``: 0 the 32-bit / f64 kernels; 1 the packed 16-bit body lane-packed
    (on ceil(ndiag / bk) lanes), 2 one pair per wavefront, 3 / 4 the same as 2 / 1 with every score times 4 (rule 3).
    ``matrix`` (packed only): None the matrix form where the scores need it (a non-simple matrix), False never, True always
    -- match / mismatch scores included; a matrix form that does not exist for the scores is an error.  ``product_variant``:
    the 32-bit / f64 variant as the planner picks it (a matrix on the fast variants), else every matrix on the generic one.
    ``want_masks``: also the decoded tie masks of every in-table cell (``mask``, the oracle's table order); ``end`` = (i, j)
    or ``ends`` = [(i, j), ..]: the same plane walked from those table cells as well (``walks``, one dict each)."""
    o = np.asarray(origin, dtype=np.int32)
    m = np.asarray(mutant, dtype=np.int32)
    if L is None:
        L = len(subst) if subst is not None else int(max([0] + list(o) + list(m))) + 1
    if subst is None:
        subst = [[match if i == j else mismatch for i in range(L)] for j in range(L)]
    S = np.ascontiguousarray(np.asarray(subst, dtype=np.float64).reshape(L, L))
    orange = origin_range if origin_range is not None else (0, len(o))
    mrange = mutant_range if mutant_range is not None else (0, len(m))
    of = np.ascontiguousarray(o[orange[0]:orange[1]])
    mf = np.ascontiguousarray(m[mrange[0]:mrange[1]])
    X, Y = len(of), len(mf)
    if X == 0:
        of = np.zeros(1, np.int32)
    if Y == 0:
        mf = np.zeros(1, np.int32)
    dr = diag_range if diag_range is not None else (0, 0)
    info = (C.c_int * 10)()
    score = C.c_double(0)
    txcap = X + Y + 2
    txbuf = C.create_string_buffer(txcap)
    hd = None
    hp = None
    if want_table:
        nd = X + Y + 1
        hd = np.zeros(nd * (min(X, Y) + 1), np.float64)
        hp = hd.ctypes.data_as(C.POINTER(C.c_double))
    lib().emu_set_waves(int(waves))
    lib().emu_set_packed_matrix(-1 if matrix is None else int(bool(matrix)))
    lib().emu_set_product_variant(int(bool(product_variant)))
    if end is not None:
        ends = [end]
    cells = _table_cells(mode, X, Y, dr)
    with _PlaneOut(cells, want_masks, ends, X, Y) as po:
        rc = lib().emu_solve(mode, alntype, of.ctypes.data_as(C.POINTER(C.c_int)), X,
                             mf.ctypes.data_as(C.POINTER(C.c_int)), Y, L,
                             S.ctypes.data_as(C.POINTER(C.c_double)), C.c_double(go), C.c_double(ge),
                             int(dr[0]), int(dr[1]), int(use_double), int(force_generic), bk,
                             info, C.byref(score), txbuf, txcap, hp, int(packed16))
    if rc != 0:
        raise ValueError('emu_solve rc=%d' % rc)
    out = dict(init_rc=info[0], opt=None, score=None, transcript=None, origin_idx=None,
               mutant_idx=None, tb_null=None, would_panick=None)
    if mode == 1:
        out['band'] = (info[1], info[2])
    if info[0] != 0:
        return out
    out['num_rows'] = info[3]
    po.fill(out, cells, orange, mrange)
    ex, ey = info[4], info[5]
    if ex < 0:
        out['opt'] = (-1, -1)
        return out
    out['opt'] = (ex, ey)
    out['score'] = score.value
    st = info[9]
    out['would_panick'] = bool(st & 4)
    out['tb_null'] = bool(st & 2) and not (st & 4)
    if not (st & 4) and not (st & 2):
        out['transcript'] = txbuf.value.decode('ascii')
        out['origin_idx'] = info[6] + orange[0]
        out['mutant_idx'] = info[7] + mrange[0]
    if want_table:
        out['hdump'] = hd
    return out


def solve_strip(origin, mutant, alntype=0, match=1., mismatch=0., go=0., ge=0., epoch=7, byte_rows=True, subst=None,
                want_masks=False, end=None, ends=None, **_):
    """Standard-mode problem through the strip pipeline (pw_strip.h): fill strip by strip, end-cell reduction, strip
    walker, fix-up.  Same result dict as :func:`solve` (``want_masks``, ``end`` / ``ends`` included)."""
    of = np.ascontiguousarray(np.asarray(origin, dtype=np.int32))
    mf = np.ascontiguousarray(np.asarray(mutant, dtype=np.int32))
    X, Y = len(of), len(mf)
    if X == 0:
        of = np.zeros(1, np.int32)
    if Y == 0:
        mf = np.zeros(1, np.int32)
    info = (C.c_int * 10)()
    score = C.c_double(0)
    txcap = X + Y + 2
    txbuf = C.create_string_buffer(txcap)
    lib().emu_set_strip_byte_rows(1 if byte_rows else 0)
    if subst is not None:
        S = np.ascontiguousarray(np.asarray(subst, dtype=np.float64))
        lib().emu_set_strip_matrix(S.ctypes.data_as(C.POINTER(C.c_double)), int(S.shape[0]))
    else:
        lib().emu_set_strip_matrix(None, 0)
    if end is not None:
        ends = [end]
    cells = (X + 1) * (Y + 1)
    with _PlaneOut(cells, want_masks, ends, X, Y) as po:
        rc = lib().emu_solve_strip(alntype, of.ctypes.data_as(C.POINTER(C.c_int)), X, mf.ctypes.data_as(C.POINTER(C.c_int)),
                                   Y, C.c_double(match), C.c_double(mismatch), C.c_double(go), C.c_double(ge),
                                   C.c_uint(epoch), info, C.byref(score), txbuf, txcap)
    if rc != 0:
        raise ValueError('emu_solve_strip rc=%d' % rc)
    out = dict(init_rc=info[0], opt=None, score=None, transcript=None, origin_idx=None,
               mutant_idx=None, tb_null=None, would_panick=None)
    if info[0] != 0:
        return out
    out['num_rows'] = info[3]
    po.fill(out, cells, (0, X), (0, Y))
    if info[4] < 0:
        out['opt'] = (-1, -1)
        return out
    out['opt'] = (info[4], info[5])
    out['score'] = score.value
    st = info[9]
    out['would_panick'] = bool(st & 4)
    out['tb_null'] = bool(st & 2) and not (st & 4)
    out['badpath'] = bool(st & 8)
    if not (st & 4) and not (st & 2):
        out['transcript'] = txbuf.value.decode('ascii')
        out['origin_idx'] = info[6]
        out['mutant_idx'] = info[7]
    return out


class NotEmulated(Exception):
    """The planner chose a kernel the emulator does not run (the tiled kernel)."""


_KERNEL = re.compile(r'^k_fill(16_mw|16|_mw|)<(int|double|)(?:, )?(\d+)(?:, (true|false))?(?:, (\d+))?')


def solve_planned(pairs, flags=0, **kw):
    """Every pair of a batch on the kernel the product's planner picks for the WHOLE batch (``batch.plan_only`` on the
    batch's shapes, with the ``PWLIB_*`` knobs of the environment): BK, lane packing, wavefronts per pair, packed rule,
    matrix form, int32 / f64, the strips, dyadic scaling.  ``pairs``: list of (origin, mutant); ``kw``: the oracle's
    scoring arguments (``mode``, ``alntype``, ``L``, ``subst`` or ``match`` / ``mismatch``, ``go``, ``ge``,
    ``diag_range`` -- one band, or a list with one per pair; ``want_masks``, ``end`` / ``ends`` as in :func:`solve`, for
    every pair).  Returns ``(plan, [result dict per pair])``.  Raises
    :class:`NotEmulated` for the tiled kernel instead of running another form."""
    from biseqt_amd.batch import plan_only
    mode, alntype = kw.get('mode', 0), kw.get('alntype', 0)
    L = kw['L']
    subst = kw.get('subst')
    if subst is None:
        subst = [[kw.get('match', 1.) if i == j else kw.get('mismatch', 0.) for i in range(L)] for j in range(L)]
    go, ge = float(kw.get('go', 0.)), float(kw.get('ge', 0.))
    dr = kw.get('diag_range')
    drs = [None] * len(pairs) if mode == 0 else ([dr] * len(pairs) if not hasattr(dr[0], '__len__') else list(dr))
    shapes = [(len(o), len(m)) + (tuple(d) if d is not None else ()) for (o, m), d in zip(pairs, drs)]
    plan = plan_only(shapes, alnmode=mode, alntype=alntype, alphabet_len=L, subst_scores=subst, go_score=go, ge_score=ge,
                     flags=flags)
    name = plan['kernel']
    if plan['tiled']:
        raise NotEmulated('the tiled kernel (%s) is not emulated' % name)
    f = float(1 << plan['scale_shift'])          # dyadic scaling: the kernels hold every score times 2^shift
    S = (np.asarray(subst, np.float64) * f).tolist()
    base = dict(mode=mode, alntype=alntype, L=L, subst=S, go=go * f, ge=ge * f, want_masks=kw.get('want_masks', False),
                end=kw.get('end'), ends=kw.get('ends'))
    out, seen = [], {}
    for (o, m), d in zip(pairs, drs):
        key = (np.asarray(o, np.int32).tobytes(), np.asarray(m, np.int32).tobytes(), d)
        if key in seen:                          # (copies of a pair, as batches that fill the chip hold: solved once)
            out.append(dict(seen[key]))
            continue
        if plan['strips']:
            if plan['strips'] != len(pairs):
                raise NotEmulated('a batch split between the strips and other kernels (%s)' % name)
            simple = all(S[i][j] == S[0][0 if i == j else 1] for i in range(L) for j in range(L)) if L > 1 else True
            byte_rows = L <= 4 and all(v == int(v) and -128 <= v <= 127 for row in S for v in row) and \
                os.environ.get('PWLIB_STRIP_NO_BYTE_ROWS', '') in ('', '0')
            r = solve_strip(o, m, alntype=alntype, match=S[0][0], mismatch=S[0][1] if L > 1 else S[0][0], go=go * f,
                            ge=ge * f, byte_rows=byte_rows, subst=None if simple else S, want_masks=base['want_masks'],
                            end=base['end'], ends=base['ends'])
        else:
            g = _KERNEL.match(name)
            if not g:
                raise NotEmulated('unknown kernel name %r' % name)
            kind, bk = g.group(1), int(g.group(3))
            waves = int(re.search(r'x (\d+) wavefronts', name).group(1)) if 'wavefronts' in name else 1
            ekw = dict(base, diag_range=d, bk=bk, waves=waves, product_variant=True)
            if kind.startswith('16'):
                x4 = plan['packed_rule'] == 3
                seg = kind == '16' and g.group(4) == 'true'
                ekw.update(packed16=(4 if x4 else 1) if seg else (3 if x4 else 2), matrix=plan['matrix'])
            else:
                ekw.update(use_double=plan['score_dtype'] == 'f64')
            r = solve(o, m, **ekw)
        if r['score'] is not None:
            r['score'] = r['score'] / f
        seen[key] = r
        out.append(dict(r))
    return plan, out
