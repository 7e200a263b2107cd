"""Strand-aware overlap discovery on the GPU.  A minus-strand pair (a, b, '-') is reads[a] against rc(reads[b]); every
answer must equal what the unchanged forward code -- and the CPU oracle -- return for (a, rc(b)) with rc(b) materialised."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COMP = np.array([3, 2, 1, 0], np.uint8)            # 'ACGT': A <-> T, C <-> G


def _rc(r):
    from biseqt_amd.sequence import reverse_complement
    return reverse_complement(r, COMP)


def _fields_equal(got, want, what):
    for name in got.dtype.names:
        if name != 'pad_':
            assert (got[name] == want[name]).all(), (what, name)


def _random_read_sets():
    """The read sets of test_overlap_gpu.test_all_pairs_random_read_sets (same generator, same draws): repeats, duplicates,
    reads shorter than the word, two-letter reads.  Yields (trial, reads, k, g_max, sensitivity)."""
    from biseqt_amd import synth
    rng = synth.rng_for(314)
    for trial in range(25):
        R = int(rng.integers(2, 22))
        k = int(rng.integers(3, 11))
        g = synth.rand_seqs(rng, 1, 1500)[0]
        reads = []
        for _ in range(R):
            kind = int(rng.integers(0, 6))
            n = int(rng.integers(0, 500))
            if kind == 0:
                reads.append(synth.rand_seqs(rng, 1, n)[0])
            elif kind == 1:
                st = int(rng.integers(0, 1500 - n)) if n < 1500 else 0
                reads.append(synth.mutate(rng, g[st:st + n], .05, .02, .3) if n else g[:0].copy())
            elif kind == 2:
                reads.append(np.resize(rng.integers(0, 4, int(rng.integers(1, 4))).astype(np.uint8), n))
            elif kind == 3 and reads:
                reads.append(reads[int(rng.integers(0, len(reads)))].copy())
            elif kind == 4:
                reads.append(rng.integers(0, 2, n).astype(np.uint8))
            else:
                reads.append(g[int(rng.integers(0, 700)):][:n].copy())
        g_max, sens = float(rng.choice([.1, .2, .3])), float(rng.choice([.9, .99]))
        yield trial, reads, k, g_max, sens


def _reference_both_strands(reads, k, g_max, sens):
    """The unchanged pair-list path over all a < b and both strands, '+' before '-', every minus T materialised: returns
    (list of (a, b, strand 0 / 1), records)."""
    from biseqt_amd.overlap import raw_bands
    R = len(reads)
    with_rc = list(reads) + [_rc(r) for r in reads]
    triples = [(a, b, s) for a in range(R) for b in range(a + 1, R) for s in (0, 1)]
    ref, _ = raw_bands(with_rc, [(a, b + R * s) for a, b, s in triples], k, 4, g_max, sens)
    return triples, ref


def test_pair_list_with_strands_equals_materialised_reverse_complements():
    from biseqt_amd import synth
    from biseqt_amd.overlap import raw_bands
    srng = synth.rng_for(2718)
    n_minus = n_seeded_minus = 0
    for trial, reads, k, g_max, sens in _random_read_sets():
        R = len(reads)
        allp = [(a, b) for a in range(R) for b in range(a + 1, R)]
        strands = ['-' if srng.integers(0, 2) else '+' for _ in allp]
        got, _ = raw_bands(reads, allp, k, 4, g_max, sens, strands=strands, complement=COMP)
        with_rc = list(reads) + [_rc(r) for r in reads]
        ref, _ = raw_bands(with_rc, [(a, b + R * (s == '-')) for (a, b), s in zip(allp, strands)], k, 4, g_max, sens)
        _fields_equal(got, ref, trial)
        minus = np.array([s == '-' for s in strands], bool)
        n_minus += int(minus.sum()); n_seeded_minus += int((ref['n_seeds'][minus] > 0).sum())
        # 0 / 1 flags are the same strands; all '+' is the unstranded call
        again, _ = raw_bands(reads, allp, k, 4, g_max, sens, strands=minus.astype(np.uint8), complement=COMP)
        _fields_equal(again, ref, trial)
        plus, _ = raw_bands(reads, allp, k, 4, g_max, sens, strands=['+'] * len(allp), complement=COMP)
        fwd, _ = raw_bands(reads, allp, k, 4, g_max, sens)
        _fields_equal(plus, fwd, trial)
    assert n_minus > 500 and n_seeded_minus > 100, (n_minus, n_seeded_minus)


def test_all_pairs_both_strands_equal_the_pair_list_over_materialised_reverse_complements():
    from biseqt_amd.overlap import raw_all_pairs
    n_listed_minus = 0
    for trial, reads, k, g_max, sens in _random_read_sets():
        triples, ref = _reference_both_strands(reads, k, g_max, sens)
        keep = [q for q, r in enumerate(ref) if r['n_seeds'] > 0]
        pairs, strand, recs, _ = raw_all_pairs(reads, k, 4, g_max, sens, strands='both', complement=COMP)
        got = [(a, b, s) for (a, b), s in zip(pairs.tolist(), strand.tolist())]
        assert got == [triples[q] for q in keep], trial
        _fields_equal(recs, ref[keep], trial)
        n_listed_minus += int(strand.sum())
        # forward only, through the new entry point: exactly the existing call
        old_pairs, old_recs, _ = raw_all_pairs(reads, k, 4, g_max, sens)
        p_pairs, p_strand, p_recs, _ = raw_all_pairs(reads, k, 4, g_max, sens, strands='+', with_strand=True)
        assert (p_pairs == old_pairs).all() and p_pairs.shape == old_pairs.shape and not p_strand.any()
        assert len(p_strand) == len(old_pairs)
        _fields_equal(p_recs, old_recs, trial)
        _fields_equal(old_recs, recs[strand == 0], trial)
        assert (old_pairs == pairs[strand == 0]).all()
        # minus only: the minus half
        m_pairs, m_strand, m_recs, _ = raw_all_pairs(reads, k, 4, g_max, sens, strands='-', complement=COMP)
        assert (m_pairs == pairs[strand == 1]).all() and m_pairs.shape == pairs[strand == 1].shape and m_strand.all()
        _fields_equal(m_recs, recs[strand == 1], trial)
    assert n_listed_minus > 100


def test_all_pairs_both_strands_shards_partition_the_work():
    """world = 3 simulated on one GPU, as test_overlap_gpu.test_all_pairs_shards_partition_the_work: disjoint shards that
    cover the unsharded list and carry the same records."""
    from biseqt_amd import synth
    from biseqt_amd.overlap import raw_all_pairs
    from tests.test_overlap_gpu import _reads
    rng = synth.rng_for(123)
    reads, _ = _reads(rng, 8000, 40, 1000, .03, .02)
    reads = [_rc(r) if q % 2 else r for q, r in enumerate(reads)]
    pairs, strand, recs, _ = raw_all_pairs(reads, 10, 4, .2, .99, strands='both', complement=COMP)
    assert strand.any() and not strand.all()
    got_p, got_s, got_r = [], [], []
    for rank in range(3):
        p, s, r, _ = raw_all_pairs(reads, 10, 4, .2, .99, rank=rank, world=3, strands='both', complement=COMP)
        assert (p[:, 0] % 3 == rank).all()
        got_p.append(p); got_s.append(s); got_r.append(r)
    gp, gs, gr = np.concatenate(got_p), np.concatenate(got_s), np.concatenate(got_r)
    assert len(gp) == len(pairs)
    order = np.lexsort((gs, gp[:, 1], gp[:, 0]))
    assert (gp[order] == pairs).all() and (gs[order] == strand).all()
    _fields_equal(gr[order], recs, 'shards')


def _stranded_reads():
    """16 reads of 1500 letters from an 8000-letter genome, each reverse-complemented with probability 1/2."""
    from biseqt_amd import synth
    rng = synth.rng_for(2024)
    g = synth.rand_seqs(rng, 1, 8000)[0]
    reads, starts, flips = [], [], []
    for _ in range(16):
        st = int(rng.integers(0, 8000 - 1500))
        r = synth.mutate(rng, g[st:st + 1500], .04, .03, .03)
        flip = bool(rng.integers(0, 2))
        reads.append(_rc(r) if flip else r); starts.append(st); flips.append(flip)
    return reads, starts, flips


def test_all_pairs_both_strands_vs_oracle_recall_and_no_false_hits():
    """Every (a, b, strand) against the oracle's highest_scoring_overlap_band(a, rc-or-not(b)); all true overlaps above 500
    letters found on their strand (33 on this input, where the oracle alone finds 33 of 33), nothing found on the wrong
    strand or between reads that do not overlap."""
    from biseqt_amd.overlap import overlap_all_pairs
    from biseqt_amd.sequence import Alphabet
    from oracle import blot_oracle as BO
    A = Alphabet('ACGT')
    reads, starts, flips = _stranded_reads()
    res = overlap_all_pairs(reads, 10, A, .2, .99, strands='both', complement=[('A', 'T'), ('C', 'G')])
    assert list(res.keys()) == sorted(res.keys(), key=lambda key: (key[0], key[1], key[2] == '-'))
    n_true = n_found = 0
    for a, b in itertools.combinations(range(16), 2):
        ov = min(starts[a], starts[b]) + 1500 - max(starts[a], starts[b])
        for strand in '+-':
            T = reads[b] if strand == '+' else _rc(reads[b])
            g = res.get((a, b, strand))
            matching = (flips[a] == flips[b]) == (strand == '+')
            if not (len(reads[a]) == len(T) and (reads[a] == T).all()):
                e = BO.highest_scoring_overlap_band(reads[a].tolist(), T.tolist(), 10, 4, .2, .99)
                assert (g is None) == (e is None), (a, b, strand)
                if e is not None:
                    assert g['d_band'] == e['d_band'] and g['len'] == e['len'], (a, b, strand, g, e)
                    assert g['p'] == e['p'] and g['score'] == e['score'], (a, b, strand, g, e)
            p = g['p'] if g is not None else 0
            if matching and ov > 500:
                n_true += 1
                assert p > .8, (a, b, strand, ov, g)
                n_found += 1
            if p > .8:
                assert matching and ov > 0, (a, b, strand, ov, g)
    assert (n_true, n_found) == (33, 33)


def test_flow_bands_then_banded_overlap_alignment_on_both_strands(oracle):
    from biseqt_amd import synth, verify
    from biseqt_amd.overlap import minus_to_forward, overlap_alignments, overlap_bands
    from biseqt_amd.sequence import Alphabet
    from tests.test_overlap_gpu import _reads
    A = Alphabet('ACGT')
    rng = synth.rng_for(4)
    reads, starts = _reads(rng, 20000, 24, 5000, .02, .02)
    flips = [q % 2 == 1 for q in range(len(reads))]
    reads = [_rc(r) if f else r for r, f in zip(reads, flips)]
    pairs, strands = [], []
    for a, b in itertools.combinations(range(len(reads)), 2):
        for s in '+-':
            pairs.append((a, b)); strands.append(s)
    bands = overlap_bands(reads, pairs, 10, A, .2, .99, strands=strands, complement=COMP)
    alns = overlap_alignments(reads, pairs, bands, A, p_min=.8, strands=strands, complement=COMP)
    true_overlap = lambda i, j: min(starts[i], starts[j]) + 5000 - max(starts[i], starts[j])
    checked = {'+': 0, '-': 0}
    for (i, j), s, band, aln in zip(pairs, strands, bands, alns):
        matching = (flips[i] == flips[j]) == (s == '+')
        if matching and true_overlap(i, j) > 800:
            assert band is not None and band['p'] > .8, (i, j, s, true_overlap(i, j), band)
            assert aln is not None and aln['strand'] == s
            T = reads[j] if s == '+' else _rc(reads[j])
            r = oracle.solve(reads[i], T, L=4, mode=1, alntype=2, diag_range=aln['diag_range'],
                             match=1, mismatch=-3, go=-5, ge=-2)
            assert aln['score'] == r['score'] and aln['transcript'] == r['transcript'], (i, j, s)
            assert (aln['origin_start'], aln['mutant_start']) == (r['origin_idx'], r['mutant_idx'])
            assert aln['score'] > 0.3 * true_overlap(i, j)
            if s == '-':
                # back to forward coordinates of reads[j]: the letters [lo, hi), read backwards and complemented, are what
                # the transcript consumed -- re-scoring it on them reproduces the score, letter for letter
                lo, hi = minus_to_forward(aln['mutant_start'], aln['transcript'], len(reads[j]))
                assert 0 <= lo < hi <= len(reads[j])
                sc, ex, ey, ok = verify.rescore(reads[i], _rc(reads[j][lo:hi]), aln['transcript'], aln['origin_start'], 0,
                                                1, -3, -5, -2)
                assert ok and sc == aln['score'] and ey == hi - lo, (i, j, sc, aln['score'])
            checked[s] += 1
        elif not matching or true_overlap(i, j) < -200:
            assert band is None or band['p'] < .8, (i, j, s)
    assert checked['-'] >= 5 and checked['+'] >= 5, checked


def test_device_arena_with_reverse_complements_and_batches_on_it():
    """The device writes the reverse complement of the reads some minus pair needs behind the letters uploaded once: those
    frames equal numpy's byte for byte, the forward frames and the slack are untouched, and batches on that shared arena
    return what a batch with a privately uploaded, materialised rc returns."""
    from biseqt_amd import _pwlib as W
    from biseqt_amd import synth
    from biseqt_amd.batch import BatchAligner, DeviceArena, pack_reads
    from biseqt_amd.overlap import aligned_batches
    rng = synth.rng_for(777)
    genome = synth.rand_seqs(rng, 1, 20000)[0]
    reads = []
    for q in range(60):
        a = int(rng.integers(0, 20000 - 1500))
        r = synth.mutate(rng, genome[a:a + int(rng.integers(600, 1500))], 0.03, 0.01, 0.5)
        reads.append(_rc(r) if q % 3 == 0 else r)
    reads += [np.zeros(0, np.uint8), np.array([2], np.uint8), np.arange(16, dtype=np.uint8) % 4, np.arange(17, dtype=np.uint8) % 4]
    arena, offs, lens = pack_reads(reads)
    which = np.array([q for q in range(len(reads)) if q % 2 == 0 or q >= 60], np.int64)
    with DeviceArena.with_reverse_complements(arena, offs, lens, which, COMP) as dev:
        back = dev.read()
        assert len(back) == dev.nbytes and dev.nbytes > arena.nbytes
        assert (back[:arena.nbytes] == arena).all()
        want = np.zeros(dev.nbytes, np.uint8)
        want[:arena.nbytes] = arena
        for q, o in zip(which.tolist(), dev.rc_offsets.tolist()):
            assert o % 16 == 0 and o >= arena.nbytes
            want[o:o + len(reads[q])] = _rc(reads[q])
        assert (back == want).all()
        assert (dev.read(int(dev.rc_offsets[1]), int(lens[which[1]])) == _rc(reads[which[1]])).all()
    # batches: pair (i, j, strand), the mutant of a minus pair is rc(reads[j])
    pidx = np.array([(i, j) for i in range(60) for j in range(i + 1, 60) if (i * 7 + j) % 9 == 0], np.int64)
    strands = ['-' if (i + j) % 2 else '+' for i, j in pidx.tolist()]
    dr = np.stack([np.maximum(-lens[pidx[:, 1]].astype(np.int64), -60), np.minimum(lens[pidx[:, 0]].astype(np.int64), 60)], axis=1)
    kw = dict(match_score=1, mismatch_score=-3, go_score=-5, ge_score=-2)
    R = len(reads)
    arena2, offs2, lens2 = pack_reads(list(reads) + [_rc(r) for r in reads])
    pidx2 = pidx.copy()
    pidx2[:, 1] += R * np.array([s == '-' for s in strands])
    with BatchAligner.from_arena(arena2, offs2, lens2, pidx2, dr, alnmode=W.BANDED_MODE, alntype=W.B_OVERLAP, alphabet_len=4, **kw) as b:
        ref = b.run().copy()
        ref_tx = b.transcripts(ref)
    got, got_tx, nb = [], [], 0
    for start, stop, b in aligned_batches(arena, offs, lens, pidx, dr, 4, max_cells=3 * 10 ** 6, strands=strands, complement=COMP, **kw):
        res = b.results()
        got.append(res.copy()); got_tx.extend(b.transcripts(res)); nb += 1
    assert nb >= 2
    got = np.concatenate(got)
    assert (got == ref).all() and got_tx == ref_tx
    assert sum(s == '-' for s in strands) > 20 and (ref['opt_i'] >= 0).any()
