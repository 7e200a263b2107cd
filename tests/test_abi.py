"""The C-ABI boundary without a GPU: the shared object loads, exports every symbol the headers
declare, the struct layouts match the reference's, and dptable_init (pure host arithmetic) agrees
with the reference on dimensions, band clamp and feasibility."""
import ctypes as C
import os
import re

import pytest

from biseqt_amd import _pwlib as W
from tests.helpers import dec, kw_of, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions(header):
    txt = open(os.path.join(ROOT, 'include', header)).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    txt = re.sub(r'//[^\n]*', '', txt)
    return set(re.findall(r'\b(dptable_\w+|pw_\w+)\s*\(', txt)) - {'pw_batch', 'pw_seed_index', 'pw_read_pair', 'pw_overlap_band'}


def test_library_loads_and_exports_every_declared_symbol():
    lib = W.load()
    declared = _declared_functions('pwlib.h') | _declared_functions('pw_batch.h')
    assert {'dptable_init', 'dptable_solve', 'dptable_traceback', 'dptable_free'} <= declared
    assert declared == set(W.EXPORTS), declared ^ set(W.EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
    seeds = _declared_functions('pw_seeds.h')
    assert seeds == set(W.SEED_EXPORTS), seeds ^ set(W.SEED_EXPORTS)
    for name in seeds:
        assert hasattr(lib, name), name
    ov = _declared_functions('pw_overlap.h')
    assert ov == set(W.OVERLAP_EXPORTS), ov ^ set(W.OVERLAP_EXPORTS)
    for name in ov:
        assert hasattr(lib, name), name
    assert C.sizeof(W.pw_read_pair) == 24


def test_struct_layouts_match_reference_abi():
    W.check_layout()     # sizeof list measured on the reference
    assert W.alnchoice.score.offset == 8 and W.alnchoice.base.offset == 16
    assert W.alnprob.mode.offset == 20 and W.alnprob.params.offset == 24
    assert W.dptable.row_lens.offset == 16 and W.dptable.prob.offset == 24
    assert W.alignment.transcript.offset == 16


def test_header_is_cdef_clean():
    """pw.py:61-66 feeds the header to cffi after dropping only lines that START with '#define'."""
    lines = open(os.path.join(ROOT, 'include', 'pwlib.h')).read().split('\n')
    kept = [l for l in lines if not l.startswith('#define')]
    assert not any(l.lstrip().startswith('#') for l in kept)


def test_enum_values_match_reference():
    assert (W.STD_MODE, W.BANDED_MODE) == (0, 1)
    assert [W.GLOBAL, W.LOCAL, W.START_ANCHORED, W.END_ANCHORED, W.OVERLAP,
            W.START_ANCHORED_OVERLAP, W.END_ANCHORED_OVERLAP] == list(range(7))
    assert [W.B_GLOBAL, W.B_LOCAL, W.B_OVERLAP] == [0, 1, 2]


def test_dptable_init_matches_reference(capfd):
    """init rc, clamped band (written back into the caller's struct), num_rows and row_lens for the
    golden problems -- dptable_init does no GPU work."""
    from oracle import ref_driver as R
    lib = R.load(W.PWLIB_SO)           # the same ctypes driver that drives the compiled reference
    recs = load_golden('random_matrix.json.gz')
    n = 0
    for k in range(0, len(recs), 3):
        rec = recs[k]
        kw = kw_of(rec)
        P = R.Problem(dec(rec['origin']), dec(rec['mutant']), **kw)
        rc = lib.dptable_init(C.byref(P.table))
        exp = rec['expect']
        assert rc == exp['init_rc'], (k, rc, exp)
        if kw['mode'] == 1:
            assert [P.params.dmin, P.params.dmax] == exp['band'], k
        if rc == 0:
            assert P.table.num_rows == exp['num_rows'], k
            X = P.frame.origin_range.j - P.frame.origin_range.i
            Y = P.frame.mutant_range.j - P.frame.mutant_range.i
            for i in range(P.table.num_rows):
                d = P.params.dmin + i if kw['mode'] == 1 else 0
                want = Y + 1 if kw['mode'] == 0 else 1 + min(d, 0) + min(X - d, Y)
                assert P.table.row_lens[i] == want
                if P.table.row_lens[i] > 0:
                    assert P.table.cells[i][0].num_choices == 0       # all cells start empty
            lib.dptable_free(C.byref(P.table))
            assert not P.table.cells
            n += 1
    assert n > 300
    C.CDLL(None).fflush(None)
    capfd.readouterr()


def test_unsupported_problems_fail_loudly(capfd):
    from oracle import ref_driver as R
    lib = R.load(W.PWLIB_SO)
    P = R.Problem([0, 1, 2], [0, 1], L=4, max_new_mins=3)
    assert lib.dptable_init(C.byref(P.table)) == -1
    # a table wider than the widest kernel (2^21 diagonals) is refused, not handed to a CPU path
    P = R.Problem([0], [0], L=4)
    P.frame.origin_range.j = 1 << 21       # only the frame lengths are read by dptable_init
    P.frame.mutant_range.j = 1 << 20
    assert lib.dptable_init(C.byref(P.table)) == -1
    # a large standard-mode table is accepted without allocating its cells on the host (lazy rows)
    P = R.Problem([0], [0], L=4)
    P.frame.origin_range.j = 100000
    P.frame.mutant_range.j = 100000
    assert lib.dptable_init(C.byref(P.table)) == 0
    assert P.table.num_rows == 100001 and P.table.row_lens[5] == 100001 and not P.table.cells[5]
    lib.dptable_free(C.byref(P.table))
    # scores that reach the reference's -INT_MAX floor of gap candidates and end cells (_pw_internals.c:267, :320, :381) are
    # refused: 50 x 45 (X + Y + 2 = 97) where one gap step lowers a score by -(ge + min(go, 0)) = 22139006 is accepted,
    # 22139007 is not; begin-anywhere types are never affected (every cell holds the begin candidate 0).  (dptable_init
    # sees the gap scores; the substitution scores of a one-diagonal band are the planner's: test_range_edges.py.)
    import numpy as np
    o = np.random.default_rng(97).integers(0, 4, 50).tolist()
    m = o[:20] + o[25:]
    for go, mode, alntype, rc in ((-22139005., 0, 0, 0), (-22139006., 0, 0, -1), (-3e9, 0, 0, -1), (-3e9, 1, 0, -1),
                                  (-3e9, 0, 1, 0), (-3e9, 0, 3, 0), (-3e9, 1, 1, 0)):
        P = R.Problem(o, m, L=4, mode=mode, alntype=alntype, match=1., mismatch=-1., go=go, ge=-1.,
                      diag_range=(-8, 8) if mode == 1 else None)
        assert lib.dptable_init(C.byref(P.table)) == rc, (go, mode, alntype)
        if rc == 0:
            lib.dptable_free(C.byref(P.table))
    C.CDLL(None).fflush(None)
    err = capfd.readouterr().err
    assert 'max_new_mins' in err and 'no CPU fallback' in err and 'INT_MAX' in err


def test_product_does_not_import_the_oracle():
    """The product path must never route through oracle/ (or the emulator)."""
    pkg = os.path.join(ROOT, 'biseqt_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(('.py', '.cpp', '.h', '.hip')):
                txt = open(os.path.join(dirpath, f)).read()
                assert 'import oracle' not in txt and 'from oracle' not in txt, f
                assert 'pw_oracle' not in txt and 'emu_wave' not in txt, f


def test_seed_and_overlap_entry_points_reject_bad_input_loudly():
    """Argument validation happens before any device work: NULL / -1 plus a message, never a silent fallback."""
    import numpy as np
    lib = W.load()
    s = np.array([0, 1, 2, 3, 0, 1], np.uint8)
    bad = np.array([0, 1, 9, 3], np.uint8)
    none = C.POINTER(C.c_uint64)()
    assert not lib.pw_seeds_create(0, s.ctypes.data, len(s), s.ctypes.data, len(s), 0, 3, none, 0, -1)
    assert b'alphabet_len' in lib.pw_seeds_last_error()
    assert not lib.pw_seeds_create(0, s.ctypes.data, len(s), s.ctypes.data, len(s), 4, 40, none, 0, -1)
    assert b'wordlen' in lib.pw_seeds_last_error()
    assert not lib.pw_seeds_create(0, s.ctypes.data, len(s), s.ctypes.data, len(s), 4, 31, none, 0, -1)
    assert b'2^62' in lib.pw_seeds_last_error()
    assert not lib.pw_seeds_create(0, bad.ctypes.data, len(bad), s.ctypes.data, len(s), 4, 3, none, 0, 0)
    assert b'letter outside the alphabet' in lib.pw_seeds_last_error()
    assert lib.pw_seeds_build(None, 0, None) == -1
    rp = (W.pw_read_pair * 1)(W.pw_read_pair(0, 4, 4, 10))          # the second read runs past the arena
    out = np.zeros(64, np.uint8)
    assert lib.pw_overlap_bands(0, s.ctypes.data, len(s), rp, 1, 4, 3, 1.1, 0.7, 1. / 64, out.ctypes.data) == -1
    assert b'outside the arena' in lib.pw_overlap_last_error()
    assert lib.pw_overlap_bands(0, s.ctypes.data, len(s), rp, 1, 4, 3, 0.0, 0.7, 1. / 64, out.ctypes.data) == -1
    assert b'coefficients' in lib.pw_overlap_last_error()
    # every refusal that comes before any device call, each with its full message
    for name, over, msg in _SEED_REFUSALS:
        _expect_refusal(lib, 'seeds', lambda: lib.pw_seeds_create(*_seeds_args(over)), msg, name)
    for name, apis, over, msg in _OVERLAP_REFUSALS:
        if 'b' in apis:
            _expect_refusal(lib, 'overlap', lambda: lib.pw_overlap_bands(*_bands_args(over)), msg, 'bands: ' + name)
        if 'a' in apis:
            _expect_refusal(lib, 'overlap', lambda: lib.pw_overlap_all_pairs(*_all_pairs_args(over)), msg, 'all pairs: ' + name)
    for name, call, msg in _NULL_INDEX_REFUSALS:
        _expect_refusal(lib, 'seeds', lambda: call(lib), msg, 'NULL index: ' + name)


def test_qseeds_refusals_before_any_device_call():
    """The query-batched index (include/pw_qseeds.h): every entry point on a NULL index, and every argument check of
    pw_qseeds_create that comes before the device is touched, each with its full message in pw_qseeds_last_error."""
    lib = W.load()
    for name, call, msg in _NULL_QINDEX_REFUSALS:
        _expect_refusal(lib, 'qseeds', lambda: call(lib), msg, 'NULL index: ' + name)
    for name, (ref, n_ref, L, k), msg in _QSEED_CREATE_REFUSALS:
        arr = None if ref is None else _arr(ref, C.c_uint8)
        n = len(ref) if n_ref is None else n_ref
        _expect_refusal(lib, 'qseeds', lambda: lib.pw_qseeds_create(0, arr, n, L, k), msg, 'pw_qseeds_create: ' + name)
    # the accessors of a NULL index that report without an error message
    assert lib.pw_qseeds_num_rows(None) == -1 and lib.pw_qseeds_num_queries(None) == -1
    assert lib.pw_qseeds_rows_device(None) is None and lib.pw_qseeds_components_rounds(None) == -1
    for ms in (lib.pw_qseeds_build_ms, lib.pw_qseeds_graph_ms, lib.pw_qseeds_components_ms, lib.pw_qseeds_count_ms):
        assert ms(None) == -1.0
    lib.pw_qseeds_destroy(None)


def test_seed_and_overlap_refusals_come_in_order():
    """With the faults of several checks at once, the first check in the library's order reports: fault i is combined
    with every later fault of the list."""
    lib = W.load()
    seeds = ['alphabet 37', 'word 32', 'masks 17', 'nS < 0', 'L^k = 2^62', 'letter in S', 'letter in T']
    bands = ['word 0', 'count < 0', 'length coefficient 0', '5^31', 'read past the arena', 'letter outside the alphabet']
    all_pairs = ['word 0', 'NULL n_out', 'length coefficient 0', 'shard world 0', '5^31', 'read past the arena',
                 'letter outside the alphabet']
    seed_table = {n: (o, m) for n, o, m in _SEED_REFUSALS}
    overlap_table = {n: (o, m) for n, _, o, m in _OVERLAP_REFUSALS}
    for api, table, order, args in (('seeds', seed_table, seeds, _seeds_args), ('overlap', overlap_table, bands, _bands_args),
                                    ('overlap', overlap_table, all_pairs, _all_pairs_args)):
        fn = {_seeds_args: lib.pw_seeds_create, _bands_args: lib.pw_overlap_bands, _all_pairs_args: lib.pw_overlap_all_pairs}[args]
        for q, name in enumerate(order):
            over = {}
            for later in reversed(order[q:]):
                over.update(table[later][0])
            _expect_refusal(lib, api, lambda: fn(*args(over)), table[name][1], '%s with every later fault' % name)


def test_seed_and_overlap_entry_points_accept_their_edges():
    """What is accepted without any device call: no pairs, fewer than two reads, and L^k = 2^62 for the overlap
    entry points (pw_seeds_create refuses the same word: its masked key is L^k itself)."""
    lib = W.load()
    for over in (dict(offs=(), lens=(), n=0), dict(L=4, k=31, offs=(), lens=(), n=0)):
        assert lib.pw_overlap_bands(*_bands_args(over)) == 0, (over, lib.pw_overlap_last_error())
        assert lib.pw_overlap_last_ms() == 0.0
    for over in (dict(offs=(), lens=(), n=0), dict(offs=(4,), lens=(6,), n=1), dict(L=4, k=31, offs=(4,), lens=(6,), n=1)):
        args = _all_pairs_args(over)
        assert args[-1][0] == 77
        assert lib.pw_overlap_all_pairs(*args) == 0, (over, lib.pw_overlap_last_error())
        assert args[-1][0] == 0 and lib.pw_overlap_last_ms() == 0.0
    _expect_refusal(lib, 'seeds', lambda: lib.pw_seeds_create(*_seeds_args(dict(L=4, k=31))),
                    b'alphabet_len ^ wordlen must be below 2^62', 'pw_seeds_create at 4^31')
    # the accessors of a NULL index that report without an error message
    assert lib.pw_seeds_num_rows(None) == -1 and lib.pw_seeds_is_self(None) == -1
    assert lib.pw_seeds_rows_device(None) is None and lib.pw_seeds_build_ms(None) == -1.0
    assert lib.pw_seeds_algorithmic_bytes(None) == -1 and lib.pw_seeds_graph_num_points(None) == -1
    lib.pw_seeds_destroy(None)


# ---- the refusal tables: keyword overrides of one valid call, listed in the order the library checks them ------------
_S = (0, 1, 2, 3, 0, 1, 2, 3)
_SEED_BASE = dict(S=_S, nS=None, T=_S, nT=None, L=4, k=3, n_masks=0, self_comp=0)
_SEED_REFUSALS = [        # pw_seeds_create: (name, overrides, message)
    ('alphabet 0', dict(L=0), b'alphabet_len must be 1..36 (kmers.py:266)'),
    ('alphabet 37', dict(L=37), b'alphabet_len must be 1..36 (kmers.py:266)'),
    ('word 0', dict(k=0), b'wordlen must be 1..31 (kmers.py:269)'),
    ('word 32', dict(k=32), b'wordlen must be 1..31 (kmers.py:269)'),
    ('masks -1', dict(n_masks=-1), b'at most 16 mask sets'),
    ('masks 17', dict(n_masks=17), b'at most 16 mask sets'),
    ('nS < 0', dict(nS=-1), b'sequence length out of range'),
    ('nT < 0', dict(nT=-1), b'sequence length out of range'),
    ('nS 2^31', dict(nS=1 << 31), b'sequence length out of range'),
    ('nT 2^31', dict(nT=1 << 31), b'sequence length out of range'),
    ('L^k = 2^62', dict(k=31), b'alphabet_len ^ wordlen must be below 2^62'),
    ('36^12', dict(L=36, k=12), b'alphabet_len ^ wordlen must be below 2^62'),
    ('letter in S', dict(S=(0, 1, 4, 3)), b'letter outside the alphabet in S'),
    ('letter in T', dict(T=(0, 1, 4, 3)), b'letter outside the alphabet in T'),
]

_READS = (0, 1, 2, 3, 0, 1, 2, 3, 3, 2)
_OVERLAP_BASE = dict(arena=_READS, offs=(0, 4), lens=(4, 6), n=None, L=4, k=3, len_coeff=1.1, radius_coeff=0.7,
                     word_p_null=1. / 64, rank=0, world=1, nulls=())
_OVERLAP_REFUSALS = [     # (name, 'b': pw_overlap_bands on the pair (read 0, read 1), 'a': pw_overlap_all_pairs, overrides, message)
    ('alphabet 0', 'ba', dict(L=0), b'alphabet_len 1..36, wordlen 1..31'),
    ('alphabet 37', 'ba', dict(L=37), b'alphabet_len 1..36, wordlen 1..31'),
    ('word 0', 'ba', dict(k=0), b'alphabet_len 1..36, wordlen 1..31'),
    ('word 32', 'ba', dict(k=32), b'alphabet_len 1..36, wordlen 1..31'),
    ('count < 0', 'ba', dict(n=-1), b'bad arguments'),
    ('2^31 reads', 'a', dict(n=1 << 31), b'bad arguments'),
    ('NULL pairs', 'b', dict(nulls=('list',)), b'bad arguments'),
    ('NULL out', 'b', dict(nulls=('out',)), b'bad arguments'),
    ('NULL read_off', 'a', dict(nulls=('read_off',)), b'bad arguments'),
    ('NULL read_len', 'a', dict(nulls=('read_len',)), b'bad arguments'),
    ('NULL n_out', 'a', dict(nulls=('n_out',)), b'bad arguments'),
    ('length coefficient 0', 'ba', dict(len_coeff=0.), b'coefficients must be positive'),
    ('radius coefficient < 0', 'ba', dict(radius_coeff=-1.), b'coefficients must be positive'),
    ('word probability NaN', 'ba', dict(word_p_null=float('nan')), b'coefficients must be positive'),
    ('shard world 0', 'a', dict(world=0), b'bad shard'),
    ('shard rank < 0', 'a', dict(rank=-1), b'bad shard'),
    ('shard rank = world', 'a', dict(rank=2, world=2), b'bad shard'),
    ('5^31', 'ba', dict(L=5, k=31), b'alphabet_len ^ wordlen must be below 2^62'),
    ('36^12', 'ba', dict(L=36, k=12), b'alphabet_len ^ wordlen must be below 2^62'),
    ('negative length', 'ba', dict(lens=(4, -1)), b'a read lies outside the arena'),
    ('read past the arena', 'ba', dict(lens=(4, 7)), b'a read lies outside the arena'),
    ('letter outside the alphabet', 'ba', dict(arena=_READS[:-1] + (4,)), b'letter outside the alphabet'),
    ('letter outside the alphabet, no reads', 'ba', dict(arena=(9,), offs=(), lens=(), n=0), b'letter outside the alphabet'),
]

_NULL_INDEX_REFUSALS = [  # (name, call on a NULL index, message)
    ('build', lambda lib: lib.pw_seeds_build(None, 0, None), b'null index'),
    ('rows', lambda lib: lib.pw_seeds_rows(None, None, 0), b'pw_seeds_rows before a successful pw_seeds_build'),
    ('count', lambda lib: lib.pw_seeds_count(None, 1, 0, 0, 0, 0, 0), b'pw_seeds_count before a successful pw_seeds_build'),
    ('kmers', lambda lib: lib.pw_seeds_kmers(None, 0, None, 0), b'null index'),
    ('band_neighbours', lambda lib: lib.pw_seeds_band_neighbours(None, None, 0, None, 0),
     b'pw_seeds_band_neighbours before a successful pw_seeds_build'),
    ('graph_build', lambda lib: lib.pw_seeds_graph_build(None, 1., 1.), b'pw_seeds_graph_build before a successful pw_seeds_build'),
    ('graph_points', lambda lib: lib.pw_seeds_graph_points(None, None, 0),
     b'pw_seeds_graph_points before a successful pw_seeds_graph_build'),
    ('graph_counts', lambda lib: lib.pw_seeds_graph_counts(None, None, 0),
     b'pw_seeds_graph_counts before a successful pw_seeds_graph_build'),
    ('graph_fetch', lambda lib: lib.pw_seeds_graph_fetch(None, None, None),
     b'pw_seeds_graph_fetch before a successful pw_seeds_graph_build'),
    ('graph_components', lambda lib: lib.pw_seeds_graph_components(None, None, None),
     b'pw_seeds_graph_components before a successful pw_seeds_graph_build'),
]

_NULL_QINDEX_REFUSALS = [  # the same for pw_qseeds_*: (name, call on a NULL index, message)
    ('build', lambda lib: lib.pw_qseeds_build(None, None, 0, 0, None, None, 0, 0, None), b'null index'),
    ('rows', lambda lib: lib.pw_qseeds_rows(None, None, 0), b'pw_qseeds_rows before a successful pw_qseeds_build'),
    ('row_offsets', lambda lib: lib.pw_qseeds_row_offsets(None, None),
     b'pw_qseeds_row_offsets before a successful pw_qseeds_build'),
    ('count_boxes', lambda lib: lib.pw_qseeds_count_boxes(None, 0, None, None, None, None, None, None),
     b'pw_qseeds_count_boxes before a successful pw_qseeds_build'),
    ('graph_build', lambda lib: lib.pw_qseeds_graph_build(None, 1., 1.), b'pw_qseeds_graph_build before a successful pw_qseeds_build'),
    ('graph_counts', lambda lib: lib.pw_qseeds_graph_counts(None, None, 0),
     b'pw_qseeds_graph_counts before a successful pw_qseeds_graph_build'),
    ('graph_fetch', lambda lib: lib.pw_qseeds_graph_fetch(None, None, None),
     b'pw_qseeds_graph_fetch before a successful pw_qseeds_graph_build'),
    ('graph_components', lambda lib: lib.pw_qseeds_graph_components(None, None, None),
     b'pw_qseeds_graph_components before a successful pw_qseeds_graph_build'),
]
_QSEED_S = (0, 1, 2, 3, 0, 1, 2, 3, 1)
_QSEED_CREATE_REFUSALS = [  # pw_qseeds_create, before any device call: (name, (ref, n_ref, L, k), message)
    ('alphabet 0', (_QSEED_S, None, 0, 3), b'alphabet_len must be 1..36 (kmers.py:266)'),
    ('alphabet 37', (_QSEED_S, None, 37, 3), b'alphabet_len must be 1..36 (kmers.py:266)'),
    ('word 0', (_QSEED_S, None, 4, 0), b'wordlen must be 1..31 (kmers.py:269)'),
    ('word 32', (_QSEED_S, None, 4, 32), b'wordlen must be 1..31 (kmers.py:269)'),
    ('L^k = 2^62', (_QSEED_S, None, 4, 31), b'alphabet_len ^ wordlen must be below 2^62'),
    ('36^12', (_QSEED_S, None, 36, 12), b'alphabet_len ^ wordlen must be below 2^62'),
    ('n_ref < 0', (_QSEED_S, -1, 4, 3), b'reference length out of range (below 2^31)'),
    ('n_ref = 2^31', (_QSEED_S, 1 << 31, 4, 3), b'reference length out of range (below 2^31)'),
    ('NULL reference', (None, 5, 4, 3), b'null reference pointer'),
    ('letter in the reference', (_QSEED_S[:-1] + (4,), None, 4, 3), b'letter outside the alphabet in the reference'),
]


def _arr(v, t):
    return (t * max(len(v), 1))(*v)


# The argument tuples hold the ctypes arrays themselves (not their addresses): they stay alive while the tuple does.
def _seeds_args(over):
    a = dict(_SEED_BASE, **over)
    return (0, _arr(a['S'], C.c_uint8), len(a['S']) if a['nS'] is None else a['nS'], _arr(a['T'], C.c_uint8),
            len(a['T']) if a['nT'] is None else a['nT'], a['L'], a['k'], _arr([0] * 17, C.c_uint64), a['n_masks'], a['self_comp'])


def _bands_args(over):
    a = dict(_OVERLAP_BASE, **over)
    pairs = (W.pw_read_pair * 1)(W.pw_read_pair(*a['offs'], *a['lens'])) if a['offs'] else None
    n = (1 if a['offs'] else 0) if a['n'] is None else a['n']
    return (0, _arr(a['arena'], C.c_uint8), len(a['arena']), None if 'list' in a['nulls'] else pairs, n, a['L'], a['k'],
            a['len_coeff'], a['radius_coeff'], a['word_p_null'], None if 'out' in a['nulls'] else _arr([0] * 64, C.c_uint8))


def _all_pairs_args(over):
    """(max_pairs = 1 and room for one record: every call here returns before the device is touched)"""
    a = dict(_OVERLAP_BASE, **over)
    n = len(a['offs']) if a['n'] is None else a['n']
    return (0, _arr(a['arena'], C.c_uint8), len(a['arena']), None if 'read_off' in a['nulls'] else _arr(a['offs'], C.c_uint64),
            None if 'read_len' in a['nulls'] else _arr(a['lens'], C.c_int32), n, a['L'], a['k'], a['len_coeff'],
            a['radius_coeff'], a['word_p_null'], a['rank'], a['world'], 1, _arr([0], C.c_int32), _arr([0], C.c_int32),
            _arr([0] * 64, C.c_uint8), None if 'n_out' in a['nulls'] else C.pointer(C.c_int64(77)))


def _expect_refusal(lib, api, call, msg, name):
    """call() fails (NULL or -1) and leaves exactly `msg` in its API's error channel.  The channel holds another
    message before the call, so a stale one cannot pass."""
    last = {'seeds': lib.pw_seeds_last_error, 'qseeds': lib.pw_qseeds_last_error, 'overlap': lib.pw_overlap_last_error,
            'batch': lib.pw_last_error}[api]
    if api == 'qseeds':
        lib.pw_qseeds_build(None, None, 0, 0, None, None, 0, 0, None)
        if last() == msg:
            lib.pw_qseeds_rows(None, None, 0)
    elif api == 'seeds':
        lib.pw_seeds_build(None, 0, None)
        if last() == msg:
            lib.pw_seeds_rows(None, None, 0)
    elif api == 'batch':
        lib.pw_plan_only(None, 0, None, 0, 0, None, 0, None)
        if last() == msg:
            lib.pw_batch_create(0, None, 0, None, 0, 0)
    else:
        lib.pw_overlap_bands(0, None, 0, None, -1, 0, 3, 1., 1., 1., None)
        if last() == msg:
            lib.pw_overlap_bands(0, None, 0, None, -1, 4, 3, 1., 1., 1., None)
    assert last() != msg
    rc = call()
    assert rc in (None, -1), (name, rc)             # NULL from pw_seeds_create / pw_batch_create, -1 from the others
    assert last() == msg, (name, last())


# ---- the batch API's refusals before any device call: pw_plan_only and the planning stage of pw_batch_create ---------
_FLOOR_MSG = (b'scores too low for this alignment type: (X + Y + 2) * (the most a gap step, or on a one-diagonal band a '
              b'substitution, can lower a score) must stay below INT_MAX, where the reference floors gap candidates and end '
              b'cells at -INT_MAX (not reproduced)')
_BATCH_BASE = dict(null_sc=False, mode=0, type=0, L=4, subst=[1. if i == j else -1. for i in range(4) for j in range(4)],
                   null_subst=False, go=-2., ge=-1., n=None, null_pairs=False, pair=dict(), arena=64, flags=0)
_BATCH_REFUSALS = [       # (name, 'c': pw_batch_create, 'p': pw_plan_only, overrides, message of create, message of plan_only)
    ('NULL scoring', 'cp', dict(null_sc=True), b'pw_batch_create: bad arguments', b'pw_plan_only: bad arguments'),
    ('count < 0', 'cp', dict(n=-1), b'pw_batch_create: bad arguments', b'pw_plan_only: bad arguments'),
    ('NULL pairs', 'cp', dict(null_pairs=True), b'pw_batch_create: bad arguments', b'pw_plan_only: bad arguments'),
    ('NULL subst', 'cp', dict(null_subst=True), b'alphabet_len must be 1..256 with a score matrix',
     b'pw_plan_only: bad arguments'),
    ('mode -1', 'cp', dict(mode=-1), b'unknown alignment mode', None),
    ('mode 2', 'cp', dict(mode=2), b'unknown alignment mode', None),
    ('type -1', 'cp', dict(type=-1), b'unknown alignment type', None),
    ('standard type 7', 'cp', dict(mode=0, type=7), b'unknown alignment type', None),
    ('banded type 3', 'cp', dict(mode=1, type=3), b'unknown alignment type', None),
    ('alphabet 0', 'cp', dict(L=0), b'alphabet_len must be 1..256 with a score matrix', None),
    ('alphabet 257', 'cp', dict(L=257), b'alphabet_len must be 1..256 with a score matrix', None),
    ('NaN score', 'cp', dict(subst=[float('nan')] + [-1.] * 15), b'substitution scores must be finite', None),
    ('infinite score', 'cp', dict(subst=[1.] * 15 + [float('inf')]), b'substitution scores must be finite', None),
    ('negative length', 'cp', dict(pair=dict(mutant_len=-1)), b'negative sequence length', None),
    ('frame outside the arena', 'cp', dict(pair=dict(origin_off=1 << 40)), b'pair frame outside the arena', None),
    ('frame one past the arena', 'cp', dict(pair=dict(mutant_off=60)), b'pair frame outside the arena', None),
    ('sequences over 2^30', 'cp', dict(arena=1 << 31, pair=dict(origin_len=(1 << 30) - 7)), b'sequences too long', None),
    ('frame off a 4-byte boundary', 'cp', dict(pair=dict(origin_off=2)), b'frames must start on a 4-byte boundary of the arena',
     None),
    ('-INT_MAX floor', 'cp', dict(go=-3e9), _FLOOR_MSG, None),
    ('score plane of a tiled pair', 'cp', dict(flags=W.PW_FLAG_DUMP_SCORES | W.PW_FLAG_FORCE_TILED),
     b'the score plane is not available for tiled (very wide) tables', None),
]


def _batch_args(over):
    """(scoring, count, pairs, arena bytes, flags) of one call; the ctypes objects stay alive while the tuple does."""
    a = dict(_BATCH_BASE, **over)
    subst = _arr(a['subst'], C.c_double)
    sc = W.pw_scoring(a['mode'], a['type'], a['L'], C.cast(subst, C.POINTER(C.c_double)) if not a['null_subst'] else None,
                      a['go'], a['ge'])
    pair = dict(dict(origin_off=0, mutant_off=16, origin_len=8, mutant_len=8, dmin=-2, dmax=2), **a['pair'])
    pairs = (W.pw_pair * 1)(W.pw_pair(*(pair[f] for f, _ in W.pw_pair._fields_)))
    return (None if a['null_sc'] else C.pointer(sc), 1 if a['n'] is None else a['n'], None if a['null_pairs'] else pairs,
            a['arena'], a['flags'], subst, sc)


def _batch_calls(lib):
    """'c': pw_batch_create on device 0, 'p': pw_plan_only, each on the arguments of _batch_args"""
    return {'c': lambda a: lib.pw_batch_create(0, *a[:5]), 'p': lambda a: lib.pw_plan_only(*a[:5], None, 0, None)}


def test_batch_api_refuses_bad_input_before_any_device_call():
    """Every refusal of pw_plan_only and of pw_batch_create's planning stage, each with its full message (both entry points
    check the same arguments; only a NULL score matrix is reported differently)."""
    lib = W.load()
    calls = _batch_calls(lib)
    for name, apis, over, msg_c, msg_p in _BATCH_REFUSALS:
        for api in apis:
            msg = msg_p if api == 'p' and msg_p is not None else msg_c
            _expect_refusal(lib, 'batch', lambda: calls[api](_batch_args(over)), msg, '%s: %s' % (api, name))
    # the edges the refusals above sit next to are accepted (planning only: no device)
    for over in (dict(), dict(L=256, subst=[0.] * (256 * 256)), dict(L=1, subst=[1.]), dict(mode=0, type=6),
                 dict(mode=1, type=2), dict(pair=dict(mutant_off=56)), dict(go=-1e6)):
        assert calls['p'](_batch_args(over)) == 0, (over, lib.pw_last_error())


def test_batch_api_refusals_come_in_order():
    """With the faults of several checks at once, the first check in the library's order reports: fault i is combined with
    every later fault of the list."""
    lib = W.load()
    calls = _batch_calls(lib)
    table = {n: (o, mc, mp) for n, _, o, mc, mp in _BATCH_REFUSALS}
    tail = ['alphabet 257', 'NaN score', 'negative length', 'frame outside the arena', 'sequences over 2^30',
            'frame off a 4-byte boundary', '-INT_MAX floor', 'score plane of a tiled pair']
    orders = {'c': ['NULL pairs', 'mode 2', 'standard type 7', 'NULL subst'] + tail,
              'p': ['NULL subst', 'mode 2', 'standard type 7'] + tail}
    for api, order in orders.items():
        for q, name in enumerate(order):
            over = {}
            for later in reversed(order[q:]):
                o = table[later][0]
                over.update(o, pair=dict(over.get('pair', {}), **o.get('pair', {})))
            msg = table[name][2] if api == 'p' and table[name][2] is not None else table[name][1]
            _expect_refusal(lib, 'batch', lambda: calls[api](_batch_args(over)), msg, '%s: %s with every later fault' % (api, name))
