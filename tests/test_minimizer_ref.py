"""The minimizer oracle itself (tests/minimizer_ref.py; no GPU): the lg / rg rule equals brute-force windows, and what follows
from the definition -- window 1 selects everything, mirror symmetry under the canonical order, the shared-substring guarantee
on both strands, a homopolymer selects every position -- then the fixtures the GPU tests lean on and the ValueErrors of the
Python arguments (raised before the library is loaded)."""
import numpy as np
import pytest

from tests import kmer_ref as KR
from tests import minimizer_ref as MR


def test_mix_is_the_stated_bijection():
    xs = [0, 1, 2, 4 ** 16 - 1, 2 ** 62, 2 ** 64 - 1, 0x9E3779B97F4A7C15]
    assert MR.mix(np.array(xs, np.uint64)).tolist() == [MR.mix_int(x) for x in xs]
    assert MR.mix_int(0) == 0xE220A8397B1DCDAF                                   # splitmix64's first output from state 0
    many = MR.mix(np.arange(100000, dtype=np.uint64))
    assert len(np.unique(many)) == len(many) and many.argmin() != 0


def test_rule_equals_brute_force_windows():
    rng = np.random.default_rng(0)
    n_sel = n_pos = 0
    for _ in range(300):
        L, k, w = int(rng.integers(1, 5)), int(rng.integers(1, 9)), int(rng.integers(1, 12))
        read = rng.integers(0, L, int(rng.integers(0, 60))).astype(np.uint8)
        comp = np.arange(L, dtype=np.uint8)[::-1].copy()
        for canonical in (False, True):
            h = MR.order_values(read, k, L, canonical, comp)
            brute, rule = MR.select_brute(h, w), MR.select_rule(h, w)
            assert np.array_equal(brute, rule), (L, k, w, read.tolist())
            assert len(h) == 0 or brute.any()
            n_sel += int(brute.sum()); n_pos += len(h)
    assert 0 < n_sel < n_pos


def test_window_one_selects_every_position_and_short_reads_get_their_minima():
    rng = np.random.default_rng(1)
    read = rng.integers(0, 4, 80).astype(np.uint8)
    assert MR.selected(read, 8, 4, 1).tolist() == list(range(73))
    k, hits = MR.table([read, read[:9]], 8, 4, 1, 'both', KR.DNA_COMPLEMENT)
    k0, hits0 = KR.table([read, read[:9]], 8, 4, 'both', KR.DNA_COMPLEMENT)
    assert np.array_equal(k, k0) and np.array_equal(hits, hits0)
    short = read[:12]                                                            # 5 positions under window 20: the minima of the 5
    h = MR.order_values(short, 8, 4)
    assert MR.selected(short, 8, 4, 20).tolist() == np.flatnonzero(h == h.min()).tolist()


def test_mirror_symmetry_under_the_canonical_order():
    rng = np.random.default_rng(2)
    for L, comp in ((4, KR.DNA_COMPLEMENT), (3, np.array([2, 1, 0], np.uint8))):
        for _ in range(40):
            k, w = int(rng.integers(1, 9)), int(rng.integers(1, 15))
            read = rng.integers(0, L, int(rng.integers(k, 90))).astype(np.uint8)
            n = len(read) - k + 1
            fwd = MR.selected(read, k, L, w, True, comp)
            rev = MR.selected(MR.revcomp(read, comp), k, L, w, True, comp)
            assert (n - 1 - fwd)[::-1].tolist() == rev.tolist()
    # and not under the plain order: a set that is not its own mirror image exists
    read = np.random.default_rng(3).integers(0, 4, 200).astype(np.uint8)
    fwd, rev = MR.selected(read, 8, 4, 10), MR.selected(MR.revcomp(read, KR.DNA_COMPLEMENT), 8, 4, 10)
    assert (193 - 1 - fwd)[::-1].tolist() != rev.tolist()


def test_shared_substring_guarantee_on_both_strands():
    rng = np.random.default_rng(4)
    for _ in range(60):
        k, w = int(rng.integers(2, 9)), int(rng.integers(1, 13))
        common = rng.integers(0, 4, w + k - 1).astype(np.uint8)
        for flip in (False, True):
            a = np.concatenate([rng.integers(0, 4, int(rng.integers(0, 40))).astype(np.uint8), common,
                                rng.integers(0, 4, int(rng.integers(0, 40))).astype(np.uint8)])
            left = rng.integers(0, 4, int(rng.integers(0, 40))).astype(np.uint8)
            b = np.concatenate([left, MR.revcomp(common, KR.DNA_COMPLEMENT) if flip else common,
                                rng.integers(0, 4, int(rng.integers(0, 40))).astype(np.uint8)])
            for strands in (('both',) if flip else ('+', 'both')):
                join = MR.sampled_join([a, b], k, 4, w, 0, strands, KR.DNA_COMPLEMENT)
                key = (0, 1, 1 if flip else 0)
                assert key in join.pairs, (k, w, flip, strands)
                # a seed inside the common stretch, on its diagonal
                d_true = [i for i in range(len(a) - len(common) + 1) if np.array_equal(a[i:i + len(common)], common)][0]
                tb = MR.revcomp(b, KR.DNA_COMPLEMENT) if flip else b
                j_true = [j for j in range(len(tb) - len(common) + 1) if np.array_equal(tb[j:j + len(common)], common)][0]
                assert (d_true - j_true) in join.pairs[key].tolist()


def test_a_homopolymer_selects_every_position():
    for letter in (0, 3):
        read = np.full(50, letter, np.uint8)
        for w in (1, 2, 7, 128):
            for canonical in (False, True):
                assert MR.selected(read, 6, 4, w, canonical, KR.DNA_COMPLEMENT).tolist() == list(range(45))


def test_density_on_random_dna_is_about_two_over_w_plus_one():
    read = np.random.default_rng(5).integers(0, 4, 60000).astype(np.uint8)
    for w, lo, hi in ((5, .32, .35), (10, .17, .19), (20, .09, .10)):
        dens = len(MR.selected(read, 16, 4, w, True, KR.DNA_COMPLEMENT)) / (60000 - 15)
        assert lo < dens < hi, (w, dens)


def test_sampled_join_at_window_one_is_the_capped_join():
    reads = KR.planted_reads(0)
    for strands in ('+', '-', 'both'):
        for cap in (0, 7):
            want = KR.capped_join(reads, KR.PLANTED_K, KR.PLANTED_L, cap, strands, KR.DNA_COMPLEMENT)
            got = MR.sampled_join(reads, KR.PLANTED_K, KR.PLANTED_L, 1, cap, strands, KR.DNA_COMPLEMENT)
            assert list(got.pairs) == list(want.pairs)
            assert all(np.array_equal(got.pairs[p], want.pairs[p]) for p in want.pairs)
            if cap:
                assert {f: got.stats[f] for f in want.stats} == want.stats
            assert got.stats['positions'] == got.stats['sampled'] == 12 * 393


def test_planted_sets_lose_rows_seeds_and_pairs_under_a_window():
    """What the GPU comparison on the planted sets can show: fewer rows, fewer seeds, a pair that changes tier or goes, and
    under cap 7 a k-mer that is masked in the sampled table."""
    reads = KR.planted_reads(1)
    full = MR.sampled_join(reads, KR.PLANTED_K, KR.PLANTED_L, 1, 0, 'both', KR.DNA_COMPLEMENT)
    for w in (2, 5, 12):
        got = MR.sampled_join(reads, KR.PLANTED_K, KR.PLANTED_L, w, 7, 'both', KR.DNA_COMPLEMENT)
        assert got.stats['sampled'] < got.stats['positions'] and got.stats['masked_entries'] > 0
        assert set(got.pairs) <= set(full.pairs)
        assert sum(map(len, got.pairs.values())) < sum(map(len, full.pairs.values()))
    assert len(got.pairs) < len(full.pairs)


def test_edge_reads_hold_what_they_claim():
    for L, k, w in ((4, 3, 16), (4, 31, 128), (36, 1, 2), (4, 16, 8)):
        reads = MR.edge_reads(L, k, w)
        n = [max(len(r) - k + 1, 0) for r in reads]
        assert n[:2] == [0, 0] and n[2:6] == [1, max(w - 1, 1), w, w + 1] and n[6:10] == [255, 256, 257, 256 + w - 1]
        assert len(set(reads[10].tolist())) == 1 and np.array_equal(reads[11][3:], reads[11][:-3])
        assert len(reads) <= 16 and max(map(len, reads)) <= 2000
    reads = MR.edge_reads(4, 5, 8)
    pal = reads[12]
    assert np.array_equal(MR.revcomp(pal, KR.DNA_COMPLEMENT), pal)
    # ties are in the fixture: the tandem repeat selects more than one position per window under w = 8
    sel = MR.selected(reads[11], 5, 4, 8, True, KR.DNA_COMPLEMENT)
    assert len(sel) > (len(reads[11]) - 4) / 8 * 2


def test_guarantee_fixture_on_the_oracle():
    """The fixture of the GPU guarantee test, confirmed on the oracle first: every pair of reads whose genome intervals overlap
    by at least w + k - 1 letters is in the sampled join on the right strand, and its true diagonal lies in the band of the
    record restated from the surviving seeds -- so a failure on the device is the device's."""
    k, w, L = MR.GUARANTEE_K, MR.GUARANTEE_W, MR.GUARANTEE_L
    reads, starts, flipped = MR.guarantee_reads()
    assert len(reads) == 10 and all(len(r) == 400 for r in reads) and any(flipped) and not all(flipped)
    truth = MR.guarantee_truth(starts, flipped, w + k - 1)
    assert len(truth) >= 8 and {s for s, _ in truth.values()} == {0, 1}
    join = MR.sampled_join(reads, k, L, w, 0, 'both', KR.DNA_COMPLEMENT)
    for (a, b), (strand, d) in truth.items():
        assert (a, b, strand) in join.pairs, (a, b, strand)
        rec = KR.band_record(join.pairs[(a, b, strand)], 400, 400, k, L)
        assert rec['d_best'] - rec['r_best'] <= d <= rec['d_best'] + rec['r_best'], (a, b, d, rec)
        # the diagonal is the true one: the letters agree along it
        T = MR.revcomp(reads[b], KR.DNA_COMPLEMENT) if strand else reads[b]
        i = np.arange(max(d, 0), min(400, 400 + d))
        assert np.array_equal(reads[a][i], T[i - d])


@pytest.mark.parametrize('bad', [-1, 129, 2.5, '5', True, [3]])
def test_a_bad_window_is_a_value_error_before_the_library_is_loaded(bad, monkeypatch):
    from biseqt_amd import _pwlib as W
    from biseqt_amd import kmers, overlap
    from biseqt_amd.sequence import Alphabet

    def no_load():
        raise AssertionError('the library was loaded before the window was checked')

    monkeypatch.setattr(W, 'load', no_load)
    reads = KR.planted_reads(0)
    with pytest.raises(ValueError, match='minimizer_window is None or an integer in 1..128'):
        overlap.raw_all_pairs(reads, 8, 4, KR.G_MAX, KR.SENSITIVITY, minimizer_window=bad)
    with pytest.raises(ValueError, match='minimizer_window is None or an integer in 1..128'):
        overlap.overlap_all_pairs(reads, 8, Alphabet('ACGT'), KR.G_MAX, KR.SENSITIVITY, minimizer_window=bad)
    with pytest.raises(ValueError, match='minimizer_window is None or an integer in 1..128'):
        overlap.raw_all_pairs_sharded(reads, 8, 4, KR.G_MAX, KR.SENSITIVITY, 0, 1, strands='both', complement=KR.DNA_COMPLEMENT,
                                      minimizer_window=bad)
    with pytest.raises(ValueError, match='window is None or an integer in 1..128'):
        kmers.KmerIndex(alphabet=Alphabet('ACGT'), wordlen=8, window=bad)
    with pytest.raises(ValueError, match='window is None or an integer in 1..128'):
        kmers.kmer_spectrum(reads, 8, Alphabet('ACGT'), window=bad)
