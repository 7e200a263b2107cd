"""The numpy reference of the k-mer table and of the capped join (tests/kmer_ref.py) against brute force, and the claims the
GPU tests rest on, shown from the reference alone (no GPU): the planted-repeat read sets have, at every cap the GPU tests
use, a k-mer exactly at the cap, one exactly above it, a pair that loses all its seeds and a pair that changes scoring tier."""
import collections
import os
import re

import numpy as np
import pytest

from biseqt_amd import _pwlib as W
from oracle import overlap_record_oracle as RO
from tests import kmer_ref as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _word(read, q, k, L):
    v = 0
    for c in read[q:q + k].tolist():
        v = v * L + int(c)
    return v


def _rc(read, comp):
    return np.asarray(comp)[np.asarray(read)[::-1]]


def test_reference_table_against_a_dict_loop():
    L, k = 4, 5
    rng = np.random.default_rng(7)
    reads = [rng.integers(0, 2, 40).astype(np.uint8) * 3 for _ in range(3)]       # two letters: plenty of repeats, palindromes
    for strands in ('+', 'both'):
        rows = []
        for strand in ((0, 1) if strands == 'both' else (0,)):
            for r, read in enumerate(reads):
                src = _rc(read, KR.DNA_COMPLEMENT) if strand else read
                for q in range(len(src) - k + 1):
                    rows.append((_word(src, q, k, L), strand, r, q))
        rows.sort()
        count = collections.Counter(key for key, _, _, _ in rows)
        keys, hits = KR.table(reads, k, L, strands, KR.DNA_COMPLEMENT)
        assert keys.tolist() == [key for key, _, _, _ in rows]
        assert hits.tolist() == [(r << 32) | (s << 31) | q for _, s, r, q in rows]
        u, c = KR.counts(reads, k, L, strands, KR.DNA_COMPLEMENT)
        assert u.tolist() == sorted(count) and c.tolist() == [count[x] for x in sorted(count)]
        mult = collections.Counter(count.values())
        top = max(mult)
        for max_mult in (1, top - 1, top, top + 3):
            want = [0] * (max_mult + 1)
            for m, n in mult.items():
                want[min(m, max_mult)] += n
            assert KR.spectrum(c, max_mult).tolist() == want
        occ = KR.occurrences(reads, k, L, strands, KR.DNA_COMPLEMENT)
        assert occ.tolist() == [count[_word(read, q, k, L)] for read in reads for q in range(len(read) - k + 1)]
        assert KR.lookup(reads, k, L, [u[0], 4 ** k, u[-1], u[0]], strands, KR.DNA_COMPLEMENT).tolist() == \
            [count[int(u[0])], 0, count[int(u[-1])], count[int(u[0])]]
        if strands == 'both':
            # count(x) = n_f(x) + n_f(rc(x)): a word that is its own reverse complement counts twice
            fwd = collections.Counter(_word(read, q, k, L) for read in reads for q in range(len(read) - k + 1))
            rc_of = {_word(w, 0, k, L): _word(_rc(w, KR.DNA_COMPLEMENT), 0, k, L)
                     for w in (np.array(RO_digits(x, k, L), np.uint8) for x in count)}
            assert all(count[x] == fwd[x] + fwd[rc_of[x]] for x in count)


def RO_digits(x, k, L):
    out = []
    for _ in range(k):
        x, c = divmod(x, L)
        out.append(c)
    return out[::-1]


def test_reference_join_against_a_dict_loop():
    L, k = 4, 4
    rng = np.random.default_rng(11)
    reads = [rng.integers(0, 4, 40).astype(np.uint8) for _ in range(3)]
    for strands in ('+', '-', 'both'):
        _, c = KR.counts(reads, k, L, '+' if strands == '+' else 'both', KR.DNA_COMPLEMENT)
        count = collections.Counter()
        for read in reads:
            for src in ((read,) if strands == '+' else (read, _rc(read, KR.DNA_COMPLEMENT))):
                count.update(_word(src, q, k, L) for q in range(len(src) - k + 1))
        for max_occ in (0, 2, int(c.max())):
            want, dropped = collections.OrderedDict(), 0
            for a in range(3):
                for b in range(a + 1, 3):
                    for strand in {'+': (0,), '-': (1,), 'both': (0, 1)}[strands]:
                        T = _rc(reads[b], KR.DNA_COMPLEMENT) if strand else reads[b]
                        rows = sorted((_word(reads[a], i, k, L), i, j) for i in range(37) for j in range(37)
                                      if _word(reads[a], i, k, L) == _word(T, j, k, L))
                        kept = [i - j for x, i, j in rows if not max_occ or count[x] <= max_occ]
                        dropped += len(rows) - len(kept)
                        if kept:
                            want[(a, b, strand)] = kept
            got = KR.capped_join(reads, k, L, max_occ, strands, KR.DNA_COMPLEMENT)
            assert list(got.pairs) == list(want)
            assert all(got.pairs[p].tolist() == want[p] for p in want)
            assert got.stats['seeds_dropped'] == dropped and got.stats['seeds_kept'] == sum(len(v) for v in want.values())
            masked = [x for x in count if max_occ and count[x] > max_occ]
            assert got.stats['distinct_masked'] == len(masked) and got.stats['masked_entries'] == sum(count[x] for x in masked)
            assert got.stats['entries'] == sum(count.values())


def test_restated_band_record_equals_the_oracle_s():
    """With the cap above the largest count nothing is masked: the record restated from a diagonal list must equal
    oracle.overlap_record_oracle.band_record on the whole pair, field for field."""
    rng = np.random.default_rng(3)
    n = 0
    for seed in KR.PLANTED_SEEDS:
        reads = KR.planted_reads(seed)
        join = KR.capped_join(reads, KR.PLANTED_K, KR.PLANTED_L, 10 ** 6)
        assert join.stats['masked_entries'] == 0 and join.stats['seeds_dropped'] == 0
        keys = list(join.pairs)
        for q in rng.permutation(len(keys))[:10]:
            a, b, _ = keys[q]
            want = RO.band_record(reads[a], reads[b], KR.PLANTED_K, KR.PLANTED_L, KR.G_MAX, KR.SENSITIVITY)
            got = KR.band_record(join.pairs[keys[q]], len(reads[a]), len(reads[b]), KR.PLANTED_K, KR.PLANTED_L)
            assert {f: got[f] for f in RO.FIELDS} == {f: want[f] for f in RO.FIELDS}, (seed, a, b)
            n += 1
    assert n == 30


def test_header_symbols_are_the_exports():
    txt = open(os.path.join(ROOT, 'include', 'pw_kmers.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    assert set(re.findall(r'\b(pw_kmers_\w+)\s*\(', txt)) == set(W.KMERS_EXPORTS)
    ov = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pw_overlap.h')).read(), flags=re.S)
    assert 'pw_overlap_all_pairs_capped' in W.OVERLAP_EXPORTS and re.search(r'\bpw_overlap_all_pairs_capped\s*\(', ov)


@pytest.mark.parametrize('seed', KR.PLANTED_SEEDS)
@pytest.mark.parametrize('max_occ', KR.PLANTED_CAPS)
def test_planted_set_earns_its_claims(seed, max_occ):
    reads = KR.planted_reads(seed)
    assert [len(r) for r in reads] == [400] * 12 + [5, 0]
    _, c = KR.counts(reads, KR.PLANTED_K, KR.PLANTED_L)
    assert (c == max_occ).any(), 'a k-mer exactly at the cap (kept)'
    assert (c == max_occ + 1).any(), 'a k-mer exactly above the cap (masked)'
    join = KR.capped_join(reads, KR.PLANTED_K, KR.PLANTED_L, max_occ)
    assert any(p not in join.pairs for p in join.uncapped), 'a pair that loses all its seeds'
    assert any(len(join.uncapped[p]) > 64 and 1 <= len(join.pairs[p]) <= 64 for p in join.pairs), 'a pair that changes tier'
    assert max_occ < join.max_count
