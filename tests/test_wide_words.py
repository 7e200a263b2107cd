"""Every input of tests/wide_words.py can tell a wrong join from a right one at its key width -- asserted on the CPU from the
oracles alone; tests/test_gpu_wide_words.py and tests/test_gpu_overlap_records.py run the same inputs on the device.  No GPU."""
import numpy as np
import pytest

from oracle import overlap_record_oracle as RO, seeds_oracle as SO
from tests import wide_words as WW

RUNGS = list(WW.LADDER)
IDS = ['L%d_k%d' % r for r in RUNGS]


def test_the_ladder_has_the_widths_it_names():
    for L, k in RUNGS:
        assert L <= 36 and k <= 31 and L ** k < 2 ** 62
        assert WW.key_bits(L, k) == WW.KEY_BITS[(L, k)] and WW.key_type(L, k) == WW.KEY_TYPE[(L, k)]
    kk = {r: r[0] ** r[1] for r in RUNGS}
    assert kk[(4, 15)] == 2 ** 30 and kk[(2, 31)] == 2 ** 31 and kk[(4, 16)] == 2 ** 32 and kk[(4, 30)] == 2 ** 60
    assert kk[(3, 20)] == 3486784401 and 2 ** 31 < kk[(3, 20)] < 0xffffffff            # the widest 4-byte key
    assert [r for r in RUNGS if WW.KEY_TYPE[r] == 32] == [(4, 15), (2, 31), (3, 20)]
    assert min(kk[r] for r in RUNGS if WW.KEY_TYPE[r] == 64) == 2 ** 32                # the first 8-byte key
    # the key widths on either side of every byte of the radix sort from the fourth on, and of the pair-id split
    assert sorted(WW.KEY_BITS.values()) == [30, 31, 32, 32, 34, 48, 57, 60, 61]
    assert [WW.pairs_per_chunk(*r) for r in ((36, 11), (4, 30), (20, 14), WW.EDGE)] == [31, 3, 1, 1]
    assert all(WW.pairs_per_chunk(*r) is None for r in RUNGS if WW.KEY_BITS[r] <= 22)
    assert WW.EDGE[0] ** WW.EDGE[1] == 2 ** 62 and WW.key_bits(*WW.EDGE) == 62
    assert set(WW.OVERLAP_RUNGS) <= set(RUNGS)


@pytest.mark.parametrize('rung', RUNGS, ids=IDS)
def test_every_input_tells_a_wrong_join_from_a_right_one(rung):
    ins = WW.inputs(*rung)
    assert {x.kind for x in ins.values()} == {'basic', 'sparse', 'empty', 'periodic', 'doubled'}
    for x in ins.values():
        assert x.S.dtype == x.T.dtype == np.uint8 and max(x.S.max(), x.T.max()) < x.alphabet_len
        WW.check_input(x)
    if rung[0] >= 32:
        assert any((x.S >= 32).any() and (x.T >= 32).any() for x in ins.values())        # letters past a 32-bit letter set


@pytest.mark.parametrize('rung', RUNGS, ids=IDS)
def test_the_variants_land_where_they_are_meant_to(rung):
    L, k = rung
    ins = WW.inputs(L, k)
    g, sens = WW.OVERLAP_RUNGS.get(rung, (.2, .99))
    rec = {name: RO.band_record(x.S, x.T, k, L, g, sens) for name, x in ins.items()}
    assert 65 <= rec['basic']['n_seeds'] <= 2048 and rec['basic']['tie'] == 1 and 0 < rec['basic']['w_best'] < 1
    assert 3 <= rec['basic']['nocc'] <= 20                 # the overlap's diagonals and those of the planted words
    assert 1 <= rec['sparse']['n_seeds'] <= 64
    assert rec['empty']['n_seeds'] == 0
    assert 2049 <= rec['periodic']['n_seeds'] <= 5000
    assert rec['two_equal_best']['tie'] == 2 and 0 < rec['two_equal_best']['w_best'] < 1
    assert abs(rec['two_equal_best']['d_best'] + 200) <= 5 and rec['two_equal_best']['d_first'] != rec['two_equal_best']['d_best']


@pytest.mark.parametrize('rung', [r for r in RUNGS if r[0] ** r[1] > 2 ** 33], ids=lambda r: 'L%d_k%d' % r)
def test_a_join_on_the_low_32_bits_counts_other_seeds(rung):
    ins = WW.inputs(*rung)
    for name in ('basic', 'sparse', 'empty'):
        x = ins[name]
        n = len(RO.seed_positions(x.S, x.T, x.wordlen, x.alphabet_len)[0])
        assert WW.count_seeds(*WW.keys(x)) == n and WW.seeds_modulo_2_32(x) > n, (rung, name)


def test_keys_at_4_16_fit_32_bits_although_the_key_type_is_64():
    x = WW.inputs(4, 16)['basic']
    assert WW.seeds_modulo_2_32(x) == WW.count_seeds(*WW.keys(x)) and WW.KEY_TYPE[(4, 16)] == 64 and 'a' not in x.planted


@pytest.mark.parametrize('rung', [(4, 15), (3, 20), (4, 16), (36, 11), (20, 14)], ids=lambda r: 'L%d_k%d' % r)
def test_the_two_cpu_oracles_agree_on_the_basic_pair(rung):
    """The int64 numpy oracle and the Python-int oracle enumerate the same rows in the same order at every width."""
    L, k = rung
    x = WW.inputs(L, k)['basic']
    i, j = RO.seed_positions(x.S, x.T, k, L)
    rows, self_comp = SO.seed_rows(x.S, x.T, k, L)
    assert not self_comp and rows == list(zip((i - j).tolist(), (i + j).tolist()))
    assert SO.as_kmer_seq(x.S.tolist(), k, L) == RO.kmer_keys(x.S, k, L).tolist()


def test_mask_sets_drop_the_zero_word_and_widen_the_sort_at_4_16():
    for L, k in RUNGS:
        x = WW.inputs(L, k)['basic']
        ks = SO.as_kmer_seq(x.S.tolist(), k, L, WW.mask_sets(L))
        assert None in ks and 0 not in ks and 0 in SO.as_kmer_seq(x.S.tolist(), k, L)
        assert (L ** k - 1 in ks) == (L != 36)                 # ({35} is the top word's letter set)
    assert (4 ** 16).bit_length() == 33 == WW.KEY_BITS[(4, 16)] + 1


def test_table_edges_sit_on_either_side_of_the_rule():
    for n, k, table in ((1008, 8, False), (1009, 8, True), (1032444, 13, False), (1032445, 13, True)):
        assert (4 ** k <= 2 ** 26 and 4 ** k // n <= 64) == table
    assert 4 ** 13 == 2 ** 26                                  # the largest table the rule admits
    for n in (1008, 1009):
        S, T = WW.table_edge_small(n)
        assert len(T) - 8 + 1 == n
        rows, sc = SO.seed_rows(S, T, 8, 4)
        assert not sc and len(rows) > 200


def test_chunk_sizes():
    assert WW.chunk_sizes(7, 4, 30) == [3, 3, 1] and WW.chunk_sizes(5, 20, 14) == [1] * 5 and WW.chunk_sizes(5, 36, 11) == [5]
    assert WW.chunk_sizes(3, *WW.EDGE) == [1, 1, 1] and WW.chunk_sizes(40, 36, 11) == [31, 9]
    assert len(WW.inputs(4, 30)) == 7 and len(WW.inputs(20, 14)) == 5


def test_nway_sets_share_rows_at_every_width():
    from tests import mseeds_ref as R
    for L, k, N in WW.NWAY:
        seqs = WW.nway(L, k, N)
        rows = R.seed_rows(seqs, k, L)
        assert len(rows) >= 50 and len(rows) < 100000
        ks = [R.kmers(s, k, L) for s in seqs]
        assert all(int(v.max()) == L ** k - 1 for v in ks)                     # the top word: every bit of the sort
        assert len({len(s) for s in seqs}) > 1
