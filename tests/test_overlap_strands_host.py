"""Strand-aware overlap discovery without a GPU: reverse complements and complement tables, the argument handling of the
stranded entry points (every refusal comes before any device call), the k-mer identity behind the reverse-strand encoder
and the map from a minus-strand alignment back to forward coordinates."""
import ctypes as C

import numpy as np
import pytest

from biseqt_amd import _pwlib as W
from biseqt_amd.sequence import Alphabet, Sequence, check_complement, complement_table, reverse_complement

ACGT = [('A', 'T'), ('C', 'G')]


def test_reverse_complement_is_an_involution_and_agrees_with_transform_and_reverse():
    A = Alphabet('ACGT')
    table = complement_table(A, ACGT)
    assert table.tolist() == [3, 2, 1, 0] and table.dtype == np.uint8
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 17, 400):
        arr = rng.integers(0, 4, n).astype(np.uint8)
        rc = reverse_complement(arr, table)
        assert rc.dtype == np.uint8 and (reverse_complement(rc, table) == arr).all()
        seq = Sequence(A, arr)
        want = seq.transform(mappings=ACGT).reverse()
        assert reverse_complement(seq, table) == want and reverse_complement(seq, ACGT) == want
        assert rc.tolist() == list(want.contents)
        assert reverse_complement(reverse_complement(seq, table), table) == seq
    assert str(reverse_complement(A.parse('AACGT'), ACGT)) == 'ACGTT'
    # letters without a rule are their own complement; a dict of one-way rules must still be an involution
    B = Alphabet('ACGTN')
    assert complement_table(B, ACGT).tolist() == [3, 2, 1, 0, 4]
    assert complement_table(B, {'A': 'T', 'T': 'A'}).tolist() == [3, 1, 2, 0, 4]


def test_complement_table_refuses_what_is_not_an_involution():
    A = Alphabet('ACGT')
    with pytest.raises(ValueError, match='its own inverse'):
        complement_table(A, {'A': 'C', 'C': 'G', 'G': 'A'})            # a permutation, but a 3-cycle
    with pytest.raises(ValueError, match='its own inverse'):
        complement_table(A, {'A': 'T'})                                 # not a permutation: T -> T
    with pytest.raises(ValueError, match='one entry per letter'):
        check_complement([3, 2, 1, 0, 4], 4)
    with pytest.raises(ValueError, match='one entry per letter'):
        check_complement([1, 0], 4)
    with pytest.raises(ValueError, match='below 4'):
        check_complement([3, 2, 1, 7], 4)
    with pytest.raises(ValueError, match='outside the alphabet'):
        reverse_complement(np.array([0, 5], np.uint8), [3, 2, 1, 0])
    assert check_complement([1, 0, 2], 3).tolist() == [1, 0, 2]


# ---- the C entry points: one valid call, overridden one fault at a time ------------------------------------------------
_READS = (0, 1, 2, 3, 0, 1, 2, 3, 3, 2)
_BASE = dict(arena=_READS, offs=(0, 4), lens=(4, 6), L=4, k=3, comp=(3, 2, 1, 0), strands=3, strand=(1,), nulls=())
_COMP_MSG = b'complement must be alphabet_len bytes with complement[complement[c]] == c for every letter'


def _arr(v, t):
    return (t * max(len(v), 1))(*v)


def _comp(a):
    return None if 'comp' in a['nulls'] else _arr(a['comp'], C.c_uint8)


def _bands_args(over):
    a = dict(_BASE, **over)
    pairs = (W.pw_read_pair * 1)(W.pw_read_pair(*a['offs'], *a['lens'])) if a['offs'] else None
    return (0, _arr(a['arena'], C.c_uint8), len(a['arena']), pairs, 1 if a['offs'] else 0, a['L'], a['k'], 1.1, 0.7, 1. / 64, _comp(a),
            _arr(a['strand'], C.c_uint8), _arr([0] * 64, C.c_uint8))


def _all_pairs_args(over):
    a = dict(_BASE, **over)
    return (0, _arr(a['arena'], C.c_uint8), len(a['arena']), _arr(a['offs'], C.c_uint64), _arr(a['lens'], C.c_int32), len(a['offs']),
            a['L'], a['k'], 1.1, 0.7, 1. / 64, _comp(a), a['strands'], 0, 1, 1, _arr([0], C.c_int32), _arr([0], C.c_int32),
            None if 'pair_strand' in a['nulls'] else _arr([0], C.c_uint8), _arr([0] * 64, C.c_uint8), C.pointer(C.c_int64(77)))


def _arena_args(over):
    a = dict(dict(_BASE, total=64, src=(0, 4), dst=(16, 32)), **over)
    return (0, _arr(a['arena'], C.c_uint8), len(a['arena']), a['total'], len(a['src']), _arr(a['src'], C.c_uint64),
            _arr(a['dst'], C.c_uint64), _arr(a['lens'], C.c_int32), _comp(a), a['L'])


_REFUSALS = [     # (name, entry points: 'b' bands, 'a' all pairs, 'u' arena upload; overrides; message)
    ('NULL complement', 'bau', dict(nulls=('comp',)), _COMP_MSG),
    ('complement that is a 3-cycle', 'bau', dict(comp=(1, 2, 0, 3)), _COMP_MSG),
    ('complement that is no permutation', 'bau', dict(comp=(3, 2, 1, 3)), _COMP_MSG),
    ('complement outside the alphabet', 'bau', dict(comp=(3, 2, 1, 4)), _COMP_MSG),
    ('strand selector 0', 'a', dict(strands=0), b'strands must be 1 (+), 2 (-) or 3 (both)'),
    ('strand selector 4', 'a', dict(strands=4), b'strands must be 1 (+), 2 (-) or 3 (both)'),
    ('strand flag 2', 'b', dict(strand=(2,)), b'strand flags must be 0 (+) or 1 (-)'),
    ('NULL pair_strand', 'a', dict(nulls=('pair_strand',)), b'bad arguments'),
    ('alphabet 37', 'ba', dict(L=37), b'alphabet_len 1..36, wordlen 1..31'),
    ('word 0', 'ba', dict(k=0), b'alphabet_len 1..36, wordlen 1..31'),
    ('read past the arena', 'bau', dict(lens=(4, 7)), b'a read lies outside the arena'),
    ('negative length', 'bau', dict(lens=(4, -1)), b'a read lies outside the arena'),
    ('letter outside the alphabet', 'bau', dict(arena=_READS[:-1] + (4,)), b'letter outside the alphabet'),
    ('rc frame inside the uploaded letters', 'u', dict(dst=(8, 32)),
     b'reverse-complement frames must ascend without overlap between the uploaded letters and total_bytes'),
    ('rc frames that overlap', 'u', dict(dst=(16, 16)),
     b'reverse-complement frames must ascend without overlap between the uploaded letters and total_bytes'),
    ('rc frame past the arena', 'u', dict(dst=(16, 60)),
     b'reverse-complement frames must ascend without overlap between the uploaded letters and total_bytes'),
    ('rc frame off a 4-byte boundary', 'u', dict(dst=(16, 30)), b'frames must start on a 4-byte boundary of the arena'),
]


def _refused(lib, call, msg, name):
    lib.pw_overlap_bands(0, None, 0, None, -1, 0, 3, 1., 1., 1., None)       # another message in the channel first
    if lib.pw_overlap_last_error() == msg:
        lib.pw_overlap_bands(0, None, 0, None, -1, 4, 3, 1., 1., 1., None)
    assert lib.pw_overlap_last_error() != msg
    rc = call()
    assert rc in (None, -1), (name, rc)
    assert lib.pw_overlap_last_error() == msg, (name, lib.pw_overlap_last_error())


def test_stranded_entry_points_refuse_bad_input_before_any_device_call():
    lib = W.load()
    for name, apis, over, msg in _REFUSALS:
        if 'b' in apis:
            _refused(lib, lambda: lib.pw_overlap_bands_stranded(*_bands_args(over)), msg, 'bands: ' + name)
        if 'a' in apis:
            _refused(lib, lambda: lib.pw_overlap_all_pairs_stranded(*_all_pairs_args(over)), msg, 'all pairs: ' + name)
        if 'u' in apis:
            _refused(lib, lambda: lib.pw_overlap_arena_upload(*_arena_args(over)), msg, 'arena: ' + name)
    _refused(lib, lambda: lib.pw_overlap_arena_read(0, None, 0, 4, None), b'bad arguments', 'arena read')


def test_stranded_entry_points_accept_their_edges():
    """No pairs and fewer than two reads return 0 without a device call, with a device time of 0; the forward-only
    selection needs no complement."""
    lib = W.load()
    assert lib.pw_overlap_bands_stranded(*_bands_args(dict(offs=(), lens=(), strand=()))) == 0, lib.pw_overlap_last_error()
    assert lib.pw_overlap_last_ms() == 0.0
    for over in (dict(offs=(), lens=()), dict(offs=(4,), lens=(6,)), dict(offs=(4,), lens=(6,), strands=1, nulls=('comp',)),
                 dict(offs=(4,), lens=(6,), strands=2)):
        args = _all_pairs_args(over)
        assert args[-1][0] == 77
        assert lib.pw_overlap_all_pairs_stranded(*args) == 0, (over, lib.pw_overlap_last_error())
        assert args[-1][0] == 0 and lib.pw_overlap_last_ms() == 0.0


def test_python_layer_refuses_bad_strands_before_the_library():
    from biseqt_amd.overlap import minus_to_forward, overlap_all_pairs, raw_all_pairs, raw_bands
    reads = [np.array([0, 1, 2, 3], np.uint8), np.array([3, 2, 1, 0, 1], np.uint8)]
    with pytest.raises(ValueError, match="'both'"):
        raw_all_pairs(reads, 3, 4, .2, .9, strands='x')
    with pytest.raises(ValueError, match='need a complement'):
        raw_all_pairs(reads, 3, 4, .2, .9, strands='both')
    with pytest.raises(ValueError, match='its own inverse'):
        raw_all_pairs(reads, 3, 4, .2, .9, strands='-', complement=[1, 2, 0, 3])
    with pytest.raises(ValueError, match='one strand per pair'):
        raw_bands(reads, [(0, 1)], 3, 4, .2, .9, strands=['+', '-'], complement=[3, 2, 1, 0])
    with pytest.raises(ValueError, match="a strand is"):
        raw_bands(reads, [(0, 1)], 3, 4, .2, .9, strands=['r'], complement=[3, 2, 1, 0])
    with pytest.raises(ValueError, match='need a complement'):
        raw_bands(reads, [(0, 1)], 3, 4, .2, .9, strands=['-'])
    with pytest.raises(ValueError, match='need a complement'):
        overlap_all_pairs(reads, 3, Alphabet('ACGT'), .2, .9, strands='both')
    with pytest.raises(AssertionError):
        minus_to_forward(3, 'MMM', 5)


@pytest.mark.parametrize('L', [2, 3, 4])
@pytest.mark.parametrize('k', [1, 3, 8, 16])
def test_reverse_strand_keys_are_the_forward_keys_of_the_materialised_reverse_complement(L, k):
    from biseqt_amd.overlap import reverse_strand_keys
    rng = np.random.default_rng(100 * L + k)
    tables = {2: [[1, 0], [0, 1]], 3: [[2, 1, 0], [0, 2, 1], [0, 1, 2]], 4: [[3, 2, 1, 0], [1, 0, 3, 2], [0, 1, 3, 2]]}[L]
    for n in (0, k - 1, k, k + 1, 50, 333):
        read = rng.integers(0, L, n).astype(np.uint8)
        for comp in tables:
            got = reverse_strand_keys(read, k, L, comp)
            rc = [comp[c] for c in read.tolist()[::-1]]                              # materialised, letter by letter
            brute = [sum(rc[j + t] * L ** (k - 1 - t) for t in range(k)) for j in range(n - k + 1)]
            assert got.dtype == np.uint64 and got.tolist() == brute, (n, comp)
            # ... and the reverse complement of the forward k-mer at len - k - j'
            fwd = [[int(c) for c in read[i:i + k]] for i in range(n - k + 1)]
            for j in range(n - k + 1):
                word = [comp[c] for c in fwd[n - k - j][::-1]]
                assert int(got[j]) == sum(w * L ** (k - 1 - t) for t, w in enumerate(word))


def test_minus_to_forward_against_brute_force():
    """Random transcripts walked op by op on T = rc(b): every position of T the path consumes is mapped letter by letter
    (j' -> len - 1 - j'); the helper's half-open interval must hold exactly those letters, and reading it backwards and
    complemented must give the letters of T the transcript consumed."""
    from biseqt_amd.overlap import minus_to_forward
    rng = np.random.default_rng(11)
    comp = np.array([3, 2, 1, 0], np.uint8)
    for trial in range(300):
        n = int(rng.integers(1, 60))
        b = rng.integers(0, 4, n).astype(np.uint8)
        T = reverse_complement(b, comp)
        j0 = int(rng.integers(0, n + 1))
        ops, j, visited = [], j0, []
        for _ in range(int(rng.integers(0, 80))):
            op = 'MSID'[int(rng.integers(0, 4))]
            if op != 'D':
                if j == n:
                    continue
                visited.append(j); j += 1
            ops.append(op)
        tx = ''.join(ops)
        lo, hi = minus_to_forward(j0, tx, n)
        fwd = sorted(n - 1 - v for v in visited)
        assert fwd == list(range(lo, hi)), (trial, tx)
        assert (lo, hi) == (n - j, n - j0)
        assert (reverse_complement(b[lo:hi], comp) == T[j0:j]).all()
        assert minus_to_forward(j0, tx.encode(), n) == (lo, hi)
