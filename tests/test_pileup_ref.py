"""The pileups without a GPU: the oracle of tests/pileup_ref.py on hand-written transcripts with hand-written expected
arrays, the ctypes structure, constants and exports of ``_pwlib`` against the text of include/pw_pileup.h, and the argument
checks of the library, ``Pileup``, ``map_queries`` and ``overlap_alignments`` that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import pileup_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    txt = open(os.path.join(ROOT, 'include', 'pw_pileup.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return re.sub(r'//[^\n]*', '', txt)


def _expect(n_cols, L, cells):
    want = R.zeros(n_cols, L)
    for (col, ch), v in cells.items():
        want[col, ch] = v
    return want


def test_oracle_on_a_transcript_with_every_special_case():
    """'IIMDIMSI' at frame start 1, origin_idx 1 (so c = 2): a leading I run counted nowhere, D directly followed by I (the
    event is anchored to the deleted column), a mutant letter >= L under 'S', a trailing I."""
    L, DEL, INS = 4, 4, 5
    counts = R.zeros(8, L)
    mutant = [3, 3, 0, 9, 1, 5, 7]           # letters 0, 1 are inserted in front; 9 and 7 are inserted letters: never read
    R.add(counts, L, 1, 6, 1, 0, 'IIMDIMSI', mutant)
    want = _expect(8, L, {(2, 0): 1, (3, DEL): 1, (3, INS): 1, (4, 1): 1, (5, INS): 1})
    assert (counts == want).all(), counts
    R.add(counts, L, 1, 6, 1, 0, 'IIMDIMSI', mutant)                   # adding is cumulative
    assert (counts == 2 * want).all()


def test_oracle_i_directly_followed_by_d_and_mutant_idx():
    L, DEL, INS = 4, 4, 5
    counts = R.zeros(3, L)
    R.add(counts, L, 0, 3, 0, 1, 'MIDM', [0, 1, 2, 3])                  # mutant_idx 1: the letters read are 1, (2), 3
    assert (counts == _expect(3, L, {(0, 1): 1, (0, INS): 1, (1, DEL): 1, (2, 3): 1})).all(), counts
    counts = R.zeros(5, L)
    R.add(counts, L, 0, 5, 0, 0, 'MIIIMDDM', [2, 0, 0, 0, 2, 1])        # an I run is ONE event; a D run counts per column
    assert (counts == _expect(5, L, {(0, 2): 1, (0, INS): 1, (1, 2): 1, (2, DEL): 1, (3, DEL): 1, (4, 1): 1})).all(), counts
    counts = R.zeros(4, L)
    R.add(counts, L, 0, 4, 0, 0, 'DIM', [3, 2])                         # a leading D: the I behind it has a column
    assert (counts == _expect(4, L, {(0, DEL): 1, (0, INS): 1, (1, 2): 1})).all(), counts


def test_oracle_pairs_that_contribute_nothing():
    L = 4
    counts = R.zeros(5, L)
    R.add(counts, L, -1, 3, 0, 0, 'MMM', [0, 1, 2])                     # a negative frame start
    R.add(counts, L, 3, 3, 0, 0, 'M', [0, 1, 2])                        # the FRAME overhangs by one column, the ops would not
    R.add(counts, L, 0, 3, 0, 0, 'MMM', [0, 1, 2], status=0)            # no traceback
    for bad in (R.ST_EMPTY, R.ST_PANICK, R.ST_BADPATH):
        R.add(counts, L, 0, 3, 0, 0, 'MMM', [0, 1, 2], status=R.ST_TRACED | bad)
    R.add(counts, L, 0, 3, 0, 0, '', [0, 1, 2])
    R.add(counts, L, 0, 3, 0, 0, None, [0, 1, 2])
    assert not counts.any()
    R.add(counts, L, 2, 3, 0, 0, 'MMM', [0, 1, 2])                      # flush with the end: it fits
    assert counts.sum() == 3 and counts[4, 2] == 1
    counts = R.zeros(3, 2)
    R.add(counts, 2, 0, 3, 0, 0, 'MBM?', [0, 1])                        # any other byte is counted nowhere and consumes nothing
    assert (counts == _expect(3, 2, {(0, 0): 1, (1, 1): 1})).all()


# L = 2: channels 0, 1, DEL, INS
CALL_ROWS = np.array([[3, 3, 0, 0],      # the two letters tie: the lower channel
                      [0, 0, 0, 0],      # nothing
                      [1, 0, 2, 0],      # DEL wins
                      [1, 1, 0, 1],      # 2 * INS == depth: no flag
                      [1, 0, 0, 1],      # 2 * INS == depth + 1: flag
                      [0, 2, 0, 0]], np.uint32)
CALL_REF = np.array([0, 0, 0, 1, 1, 0], np.uint8)


def test_oracle_call_tie_rule_and_min_depth():
    def rows(s):
        return [(int(r['depth']), int(r['call']), int(r['ref']), int(r['flags'])) for r in s]
    assert rows(R.call(CALL_ROWS, 2, None, 1)) == [(6, 0, 255, 1), (0, 255, 255, 0), (3, 2, 255, 1), (2, 0, 255, 1), (1, 0, 255, 5),
                                                   (2, 1, 255, 1)]
    assert rows(R.call(CALL_ROWS, 2, CALL_REF, 1)) == [(6, 0, 0, 1), (0, 255, 0, 0), (3, 2, 0, 3), (2, 0, 1, 3), (1, 0, 1, 7), (2, 1, 0, 3)]
    assert rows(R.call(CALL_ROWS, 2, CALL_REF, 3)) == [(6, 0, 0, 1), (0, 255, 0, 0), (3, 2, 0, 3), (2, 255, 1, 0), (1, 255, 1, 0),
                                                       (2, 255, 0, 0)]
    assert len(R.call(R.zeros(0, 2), 2)) == 0


def test_site_structure_layout():
    from biseqt_amd import _pwlib as W
    from biseqt_amd import batch as B
    assert C.sizeof(W.pw_pileup_site) == 8
    assert [(f, getattr(W.pw_pileup_site, f).offset, getattr(W.pw_pileup_site, f).size) for f, _ in W.pw_pileup_site._fields_] == \
        [('depth', 0, 4), ('call', 4, 1), ('ref', 5, 1), ('flags', 6, 2)]
    W.check_layout()
    assert W.SIZEOF['pw_pileup_site'] == 8
    for dt in (B.SITE_DTYPE, R.SITE_DTYPE):
        assert dt.itemsize == 8 and [(n, dt.fields[n][1]) for n in dt.names] == [('depth', 0), ('call', 4), ('ref', 5), ('flags', 6)]


def test_constants_and_exports_match_the_header():
    from biseqt_amd import _pwlib as W
    lib = W.load()
    txt = _header()
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define\s+(PW_PILEUP_\w+)\s+(\d+)\b', txt)}
    assert defines == dict(PW_PILEUP_COVERED=1, PW_PILEUP_DIFFERS=2, PW_PILEUP_INSERT=4), defines
    for name, value in defines.items():
        assert getattr(W, name) == value, name
    assert (R.COVERED, R.DIFFERS, R.INSERT) == (W.PW_PILEUP_COVERED, W.PW_PILEUP_DIFFERS, W.PW_PILEUP_INSERT)
    assert re.search(r'#define\s+PW_PILEUP_DEL\(L\)\s+\(L\)', txt) and re.search(r'#define\s+PW_PILEUP_INS\(L\)\s+\(\(L\)\s*\+\s*1\)', txt)
    declared = set(re.findall(r'\b(pw_\w+)\s*\(', txt))
    assert declared == set(W.PILEUP_EXPORTS), declared ^ set(W.PILEUP_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert re.search(r'typedef struct \{ uint32_t depth; uint8_t call; uint8_t ref; uint16_t flags; \} pw_pileup_site;', txt)


def test_library_refuses_bad_arguments_before_any_device_call():
    from biseqt_amd import _pwlib as W
    lib = W.load()
    for L in (0, 33, -1):
        assert not lib.pw_pileup_create(0, 5, L) and 'alphabet_len must be 1..32' in W.last_error()
    assert not lib.pw_pileup_create(0, -1, 4) and 'n_cols' in W.last_error()
    out = np.zeros(8, np.uint32)
    assert lib.pw_pileup_clear(None, None) == -1 and 'null pileup' in W.last_error()
    assert lib.pw_pileup_counts(None, 0, 1, out.ctypes.data) == -1 and 'null pileup' in W.last_error()
    assert lib.pw_pileup_set_counts(None, 0, 1, out.ctypes.data) == -1 and 'null pileup' in W.last_error()
    assert lib.pw_pileup_call(None, None, 1, None) == -1 and 'null pileup' in W.last_error()
    assert lib.pw_pileup_sites(None, 0, 1, out.ctypes.data) == -1 and 'null pileup' in W.last_error()
    assert lib.pw_batch_pileup_add(None, None, None, 0, None) == -1 and 'null batch or pileup' in W.last_error()
    assert not lib.pw_pileup_counts_device(None) and not lib.pw_pileup_sites_device(None)
    lib.pw_pileup_destroy(None)


def test_python_argument_validation_needs_no_device():
    from biseqt_amd.batch import Pileup
    from biseqt_amd.overlap import overlap_alignments
    from biseqt_amd.pipeline import map_queries
    from biseqt_amd.sequence import Alphabet, Sequence
    for L in (0, 33):
        with pytest.raises(ValueError, match='alphabet_len'):
            Pileup(10, L)
    with pytest.raises(ValueError, match='n_cols'):
        Pileup(-1, 4)
    A = Alphabet('ACGT')
    ref, q = Sequence(A, (0, 1, 2, 3) * 10), Sequence(A, (0, 1, 2, 3) * 5)
    args = (ref, [q], 10, .8, 6, .2, .9)
    with pytest.raises(ValueError, match="'best' or 'all'"):
        map_queries(*args, pileup_records='first')
    with pytest.raises(ValueError, match='open biseqt_amd.batch.Pileup'):
        map_queries(*args, pileup=np.zeros((40, 6), np.uint32))
    with pytest.raises(ValueError, match='open biseqt_amd.batch.Pileup'):
        overlap_alignments([ref, q], [(0, 1)], [None], A, pileup=object())


def test_best_record_rule_of_map_queries():
    """pipeline.pileup_col0: per query the record with an alignment and the highest score, a tie to the earlier one."""
    from biseqt_amd.batch import RESULT_DTYPE
    from biseqt_amd.pipeline import pileup_col0
    res = np.zeros(8, RESULT_DTYPE)
    res['score'] = [5, 7, 7, 9, 3, 1, 2, 2]
    res['opt_i'] = [1, 1, 1, -1, 1, 1, 1, 1]
    res['tx_len'] = [4, 4, 4, 4, 0, 4, 4, 4]
    # query 0: records 0..2 (7 ties: the earlier), query 1: none, query 2: record 3 has no end cell, 4 no transcript: nothing,
    # query 3: records 5..7 (2 ties: the earlier)
    assert pileup_col0(res, [3, 0, 2, 3], 'best').tolist() == [-1, 0, -1, -1, -1, -1, 0, -1]
    assert pileup_col0(res, [3, 0, 2, 3], 'all').tolist() == [0, 0, 0, -1, -1, 0, 0, 0]
    assert pileup_col0(res[:0], [], 'best').tolist() == []
