"""Cases of tests/test_gpu_polish_add.py that need no device to be built: GLOBAL pairs whose transcripts have chosen lengths
and gap runs at chosen places, and the oracle's two-sided pileup of a batch."""
import numpy as np

from tests import polish_ref as PR

# gaps cheaper than a substitution: under these scores the optimal GLOBAL alignment of a constructed pair is the construction
GAPPY = dict(match_score=1, mismatch_score=-20, go_score=-2, ge_score=-1)
SCAN_LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 258, 259, 511, 512, 513)
RUN_LENGTHS = (1, 2, 3, 8, 9)            # 1, J and J + 1 for J = 2 and J = 8


def pair_of_ops(rng, ops):
    """(origin, mutant) whose alignment column by column is ``ops`` (M, I, D).  No gap block can slide: its first letter
    differs from the letter behind the block, its last one from the letter in front of it."""
    n = len(ops)
    u = rng.integers(0, 4, n).astype(np.uint8)
    k = 0
    while k < n:
        if ops[k] == 'M':
            k += 1
            continue
        s = k
        while k < n and ops[k] == ops[s]:
            k += 1
        left = {int(u[s - 1])} if s > 0 else set()
        right = {int(u[k])} if k < n else set()
        if k - s == 1:
            u[s] = min(set(range(4)) - left - right)
        else:
            u[s], u[k - 1] = min(set(range(4)) - right), min(set(range(4)) - left)
    cols = np.array(list(ops))
    return u[cols != 'I'].copy(), u[cols != 'D'].copy()


def scan_ops():
    """The column strings: every length of SCAN_LENGTHS; from 63 ops on an inner run of I or of D of every RUN_LENGTHS at
    places around the dword, lane and 256-byte edges, between a leading and a trailing gap of either kind."""
    out = ['M', 'IM', 'MD', 'DMI', 'IMD', 'DMMI', 'IMMD', 'IMIMD', 'DMDMI']
    # a replaced letter aligns as a run directly followed by a run of the other kind
    out += ['MMMIDMMM', 'MMDIMM', 'M' * 30 + 'IID' + 'M' * 31, 'M' * 29 + 'DDI' + 'M' * 33, 'M' * 252 + 'IIDD' + 'M' * 9,
            'M' * 253 + 'DIII' + 'M' * 250]
    ends = ('ID', 'DI', 'II', 'DD')
    q = 0
    for n in SCAN_LENGTHS[5:]:
        starts = (29, 30, 31, 32) if n < 255 else (n - 12, n - 11, n - 10, 251, 252, 253, 254)[:4 if n < 260 else 7]
        for kind in 'ID':
            for run in RUN_LENGTHS:
                for s in starts:
                    if s < 2 or s + run > n - 2:
                        continue
                    lead, trail = ends[q % 4]
                    q += 1
                    out.append(lead + 'M' * (s - 1) + kind * run + 'M' * (n - s - run - 1) + trail)
    return out


def scan_pairs(seed=7701):
    rng = np.random.default_rng(seed)
    return [pair_of_ops(rng, ops) for ops in scan_ops()]


def gap_runs(tx, op):
    runs, k = [], 0
    while k < len(tx):
        if tx[k] == op:
            s = k
            while k < len(tx) and tx[k] == op:
                k += 1
            runs.append((s, k))
        else:
            k += 1
    return runs


def expected(n_cols, L, J, res, txs, geo, sides, ocol0=None, mcol0=None, rev=None, comp=None, arena_first=0):
    """The oracle's pileup of a batch.  ``geo[k]`` = (origin_off, mutant_off, origin letters, mutant letters) of pair k, the
    letters as the batch's frames hold them (for a reversed pair the mutant letters are those of the reverse complement)."""
    counts, ins = PR.zeros(n_cols, L, J)
    for k, tx in enumerate(txs):
        if not tx:
            continue
        o_off, m_off, o, m = geo[k]
        st, oi, mi = int(res['status'][k]), int(res['origin_idx'][k]), int(res['mutant_idx'][k])
        if sides & 1:
            f = int(ocol0[k]) if ocol0 is not None else o_off - arena_first
            PR.add(counts, ins, L, f, len(o), oi, mi, tx, m, st)
        if sides & 2:
            f = int(mcol0[k]) if mcol0 is not None else m_off - arena_first
            if rev is not None and rev[k]:
                PR.add_mutant_side_reversed(counts, ins, L, f, o, len(m), oi, mi, tx, comp, st)
            else:
                PR.add_mutant_side(counts, ins, L, f, o, len(m), oi, mi, tx, st)
    return counts, ins
