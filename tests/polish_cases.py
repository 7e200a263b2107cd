"""The fixture of the correction experiment, shared by tests/test_polish_ref.py (CPU oracle) and
tests/test_gpu_polish_reads.py (device): synthetic reads of both strands with known positions, the true overlaps as pairs,
and bands around the true diagonals.  Also the oracle's pileup of a list of alignments, both sides, minus pairs reversed."""
import numpy as np

from tests import polish_ref as PR

L = 4
COMPLEMENT = np.array([3, 2, 1, 0], np.uint8)
SCORES = dict(match_score=1, mismatch_score=-3, go_score=-5, ge_score=-2)
GENOME, N_READS, READ_LEN, MIN_OVERLAP, BAND = 1500, 45, 400, 150, 40
P_SUBST, P_INS, P_DEL = .03, .02, .02
MIN_DEPTH, INS_SLOTS, SELF_WEIGHT = 3, 2, 1


def rc(a):
    return COMPLEMENT[np.asarray(a, np.uint8)[::-1]]


def noisy(rng, src):
    out = []
    for x in src:
        if rng.random() >= P_DEL:
            out.append(int((x + rng.integers(1, L)) % L) if rng.random() < P_SUBST else int(x))
        if rng.random() < P_INS:
            out.append(int(rng.integers(0, L)))
    return np.array(out, np.uint8)


_cache = {}


def fixture(seed=7601, n_reads=N_READS, genome_len=GENOME):
    """dict(reads, truth, pairs, strands, bands): ``truth[r]`` is the error-free source of read r in the read's own
    orientation; pair ``(a, b)`` with strand '-' aligns reads[a] with rc(reads[b]); ``bands[q]['d_band']`` is +-BAND around the
    true diagonal of pair q in that frame."""
    key = (seed, n_reads, genome_len)
    if key in _cache:
        return _cache[key]
    rng = np.random.Generator(np.random.PCG64(seed))
    genome = rng.integers(0, L, genome_len, dtype=np.uint8)
    starts = rng.integers(0, genome_len - READ_LEN + 1, n_reads)
    minus = rng.random(n_reads) < .5
    reads, truth = [], []
    for p, neg in zip(starts.tolist(), minus.tolist()):
        src = genome[p:p + READ_LEN]
        src = rc(src) if neg else src
        truth.append(np.ascontiguousarray(src))
        reads.append(noisy(rng, src))
    pairs, strands, bands = [], [], []
    for a in range(n_reads):
        for b in range(a + 1, n_reads):
            if READ_LEN - abs(int(starts[a]) - int(starts[b])) < MIN_OVERLAP:
                continue
            # in the orientation of read a, read b (turned the same way) starts d letters behind the start of read a
            d = int(starts[b]) - int(starts[a])
            if minus[a]:
                d = -d
            pairs.append((a, b))
            strands.append('+' if minus[a] == minus[b] else '-')
            bands.append(dict(d_band=(d - BAND, d + BAND), p=1.))
    _cache[key] = dict(reads=reads, truth=truth, pairs=pairs, strands=strands, bands=bands)
    return _cache[key]


def total_distance(reads, truth):
    return sum(PR.edit_distance(r, t) for r, t in zip(reads, truth))


def pileup_of(reads, offs, n_cols, pairs, strands, alns, J, self_weight):
    """The oracle's pileup: the self vote of every read, and every alignment of ``alns`` (None, or a dict with transcript,
    origin_start, mutant_start; a minus pair in the frame of rc(reads[b])) added onto both of its reads."""
    counts, ins = PR.zeros(n_cols, L, J)
    for r, off in zip(reads, offs):
        PR.add_letters(counts, L, r, int(off), self_weight)
    for (a, b), st, aln in zip(pairs, strands, alns):
        if aln is None or not aln['transcript']:
            continue
        t, oi, mi = aln['transcript'], aln['origin_start'], aln['mutant_start']
        mutant = rc(reads[b]) if st == '-' else reads[b]
        PR.add(counts, ins, L, int(offs[a]), len(reads[a]), oi, mi, t, mutant)
        if st == '-':
            PR.add_mutant_side_reversed(counts, ins, L, int(offs[b]), reads[a], len(reads[b]), oi, mi, t, COMPLEMENT)
        else:
            PR.add_mutant_side(counts, ins, L, int(offs[b]), reads[a], len(reads[b]), oi, mi, t)
    return counts, ins


def oracle_alignments(oracle, fx):
    """B_OVERLAP alignments of the fixture's pairs by the CPU oracle, as overlap_alignments reports them."""
    key = ('alns', id(fx))
    if key in _cache:
        return _cache[key]
    out = []
    for (a, b), st, band in zip(fx['pairs'], fx['strands'], fx['bands']):
        S, T = fx['reads'][a], fx['reads'][b]
        T = rc(T) if st == '-' else T
        lo, hi = max(band['d_band'][0], -len(T)), min(band['d_band'][1], len(S))
        r = oracle.solve(S, T, mode=oracle.BANDED_MODE, alntype=oracle.B_OVERLAP, L=L, match=1, mismatch=-3, go=-5, ge=-2,
                         diag_range=(lo, hi))
        out.append(None if not r.get('transcript') else
                   dict(transcript=r['transcript'], origin_start=r['origin_idx'], mutant_start=r['mutant_idx']))
    _cache[key] = out
    return out
