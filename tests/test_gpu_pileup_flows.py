"""Pileups through the two flows (``pipeline.map_queries(pileup=...)``, ``overlap.overlap_alignments(pileup=...)``) against the
oracle of tests/pileup_ref.py applied to the alignments the flows return to the host: counts compared with ``==``."""
import numpy as np
import pytest

from tests import blot_many_cases as Cs
from tests import pileup_ref as R

pytestmark = pytest.mark.gpu
COMP = [('A', 'T'), ('C', 'G')]
L = 4


def _rc(a):
    return (3 - np.asarray(a, np.uint8))[::-1].copy()            # ACGT = 0123: A <-> T, C <-> G


PLANTED = (300, 700, 1000, 1400, 1700)


@pytest.fixture(scope='module')
def mapping():
    """A 2 kb reference; the reads' source is the reference with five substitutions planted; 60 exact reads of 120 letters
    tile the source evenly (3 to 4 deep), every odd one given reverse-complemented."""
    from biseqt_amd import synth
    rng = synth.rng_for(7601)
    ref = synth.rand_seqs(rng, 1, 2000)[0]
    source = ref.copy()
    for x in PLANTED:
        source[x] = (source[x] + 1) % 4
    starts = [round(k * (2000 - 120) / 59) for k in range(60)]
    reads = [source[s:s + 120].copy() for s in starts]
    reads = [_rc(r) if k % 2 else r for k, r in enumerate(reads)]
    return ref, source, reads


def _aligned(rec):
    aln = rec['alignment']
    return (rec['segment'], rec['p'], rec['diag_range'], rec['score'], rec['p_aln'], rec['len_aln'], rec['strand'], rec['query_interval'],
            None if aln is None else (aln.transcript, aln.origin_start, aln.mutant_start))


def _oracle_of_records(mapped, reads, n_cols, which):
    counts = R.zeros(n_cols, L)
    n = 0
    for q, recs in enumerate(mapped):
        chosen = [r for r in recs if r['alignment'] is not None]
        if which == 'best' and chosen:
            best = chosen[0]
            for r in chosen[1:]:                                  # the highest score; a tie goes to the earlier record
                if r['score'] > best['score']:
                    best = r
            chosen = [best]
        for r in chosen:
            aln = r['alignment']
            T = _rc(reads[q]) if r['strand'] == '-' else reads[q]
            R.add(counts, L, 0, n_cols, aln.origin_start, aln.mutant_start, aln.transcript, T)
            n += 1
    return counts, n


def test_map_queries_pileup(mapping):
    from biseqt_amd import _pwlib as W
    from biseqt_amd.batch import Pileup
    from biseqt_amd.pipeline import map_queries
    ref, source, reads = mapping
    Rf, Q = Cs.mk(ref), [Cs.mk(t) for t in reads]
    args = (60, .7, 8, Cs.G_MAX, Cs.SENS)
    kw = dict(keep=3, strands='both', complement=COMP)
    plain_full = map_queries(Rf, Q, *args, **kw)
    plain_lean = map_queries(Rf, Q, *args, alignments=False, **kw)
    with Pileup(len(ref), L) as p_lean, Pileup(len(ref), L) as p_full, Pileup(len(ref), L) as p_all:
        lean = map_queries(Rf, Q, *args, alignments=False, pileup=p_lean, **kw)
        full = map_queries(Rf, Q, *args, pileup=p_full, cigar='extended', **kw)
        every = map_queries(Rf, Q, *args, alignments=False, pileup=p_all, pileup_records='all', **kw)
        # the function returns what it returns without a pileup
        assert lean == plain_lean == every
        assert [[_aligned(r) for r in recs] for recs in full] == [[_aligned(r) for r in recs] for recs in plain_full]
        want, n_best = _oracle_of_records(plain_full, reads, len(ref), 'best')
        want_all, n_all = _oracle_of_records(plain_full, reads, len(ref), 'all')
        assert n_best >= 50 and n_all >= n_best
        assert {r['strand'] for recs in plain_full for r in recs if r['alignment'] is not None} == {'+', '-'}
        got = p_lean.counts()
        assert (got == want).all(), np.argwhere(got != want)[:8]
        assert (p_full.counts() == want).all()
        assert (p_all.counts() == want_all).all()
        # the planted substitutions show up, and the consensus is the reads' source wherever three reads cover it
        p_lean.call(ref=ref, min_depth=3)
        sites, osites = p_lean.sites(), R.call(want, L, ref, 3)
        for f in ('depth', 'call', 'ref', 'flags'):
            assert (sites[f] == osites[f]).all(), f
        deep = osites['depth'] >= 3
        assert deep.sum() >= 1500 and all(deep[x] for x in PLANTED)
        assert (osites['call'][deep] == source[deep]).all()              # ... holds for the oracle
        assert (p_lean.consensus()[deep] == source[deep]).all()
        assert (p_lean.consensus(100, 900) == p_lean.consensus()[100:900]).all()
        ovars = np.flatnonzero(osites['flags'] & (W.PW_PILEUP_DIFFERS | W.PW_PILEUP_INSERT)).tolist()
        assert ovars == list(PLANTED)
        assert p_lean.variants().tolist() == ovars and p_lean.variants(500, 1500).tolist() == [700, 1000, 1400]
        # the pileup is the caller's: a second call adds to it
        map_queries(Rf, Q, *args, alignments=False, pileup=p_lean, **kw)
        assert (p_lean.counts() == 2 * want).all()
    with Pileup(len(ref) + 1, L) as bad, pytest.raises(ValueError, match='n_cols == len'):
        map_queries(Rf, Q, *args, pileup=bad, **kw)
    with Pileup(len(ref), 5) as bad, pytest.raises(ValueError, match='alphabet_len'):
        map_queries(Rf, Q, *args, pileup=bad, **kw)


def _batch_count(lens, pairs, dr, max_cells):
    """The batches overlap.aligned_batches cuts: at most max_cells cells each, at least one pair."""
    cells = [(hi - lo + 1) * min(int(lens[i]), int(lens[j])) for (i, j), (lo, hi) in zip(pairs, dr)]
    n, acc = 1, 0
    for k, c in enumerate(cells):
        if acc and acc + c > max_cells:
            n, acc = n + 1, 0
        acc += c
    return n


def test_overlap_alignments_pileup():
    from biseqt_amd import synth
    from biseqt_amd.batch import Pileup, pack_reads
    from biseqt_amd.overlap import overlap_alignments
    from biseqt_amd.sequence import Alphabet
    rng = synth.rng_for(7602)
    genome = synth.rand_seqs(rng, 1, 1500)[0]
    flipped = [k % 3 == 1 for k in range(12)]
    reads = []
    for k in range(12):
        w = synth.mutate(rng, genome[100 * k:100 * k + 400], 0.03, 0.01, 0.2)
        reads.append(_rc(w) if flipped[k] else w)
    arena, offs, lens = pack_reads(reads)
    pairs, bands, strands, dr = [], [], [], []
    for i in range(12):
        for j in (i + 1, i + 2):
            if j >= 12:
                continue
            # the diagonal of the overlap in the frame of reads[i] as given (a flipped origin turns the shift around)
            d = -100 * (j - i) + (int(lens[i]) - int(lens[j])) if flipped[i] else 100 * (j - i)
            pairs.append((i, j)); strands.append('-' if flipped[i] != flipped[j] else '+')
            bands.append(dict(p=1., d_band=(d - 25, d + 25)))
            dr.append((max(d - 25, -int(lens[j])), min(d + 25, int(lens[i]))))
    max_cells = 130000
    assert _batch_count(lens, pairs, dr, max_cells) >= 3 and '-' in strands and '+' in strands
    A = Alphabet('ACGT')
    kw = dict(device=0, max_cells=max_cells, strands=strands, complement=COMP)
    with Pileup(arena.nbytes, L) as p, Pileup(arena.nbytes, L) as p_lean:
        alns = overlap_alignments(reads, pairs, bands, A, pileup=p, **kw)
        lean = overlap_alignments(reads, pairs, bands, A, pileup=p_lean, want_transcripts=False, **kw)
        assert alns == overlap_alignments(reads, pairs, bands, A, **kw)
        want = R.zeros(arena.nbytes, L)
        n = 0
        for (i, j), a in zip(pairs, alns):
            if a is None:
                continue
            T = _rc(reads[j]) if a['strand'] == '-' else reads[j]
            R.add(want, L, int(offs[i]), int(lens[i]), a['origin_start'], a['mutant_start'], a['transcript'], T)
            n += bool(a['transcript'])
        assert n >= 18, n
        got = p.counts()
        assert (got == want).all(), np.argwhere(got != want)[:8]
        assert (p_lean.counts() == want).all()
        assert [None if a is None else a['score'] for a in lean] == [None if a is None else a['score'] for a in alns]
        # a read's columns are [offs[r], offs[r] + lens[r]); the padding between two reads stays zero
        inside = np.zeros(arena.nbytes, bool)
        for r in range(12):
            inside[offs[r]:offs[r] + lens[r]] = True
            if r < 10:
                assert p.counts(int(offs[r]), int(offs[r] + lens[r]))[:, :5].sum() > 0, r
        assert not got[~inside].any() and got[inside].any()
    with Pileup(arena.nbytes - 1, L) as bad, pytest.raises(ValueError, match='span the arena'):
        overlap_alignments(reads, pairs, bands, A, pileup=bad, **kw)
