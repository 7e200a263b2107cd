"""Seeded read sets with their true overlaps, as records for tests/graph_ref.py and ``OverlapGraph.add``: rows
``(a, b, strand, a_beg, a_end, b_beg, b_end, n_match, n_ops)`` with ``a < b``.  Every read is a stretch of a genome, stored
forwards (orientation 0) or reverse-complemented (orientation 1); the reads are error-free, so ``n_match == n_ops``."""
import numpy as np

COMPLEMENT = np.array([3, 2, 1, 0], np.uint8)


def rc(letters):
    return COMPLEMENT[np.asarray(letters, np.uint8)[::-1]]


def _record(a, b, oa, ob, la, lb, ia, ib):
    """The record of reads ``a < b`` whose forward versions overlap in ``ia`` (on a) and ``ib`` (on b): the frame is read a as
    stored and read b turned into a's orientation."""
    if oa:
        ia, ib = (la - ia[1], la - ia[0]), (lb - ib[1], lb - ib[0])
    n = ia[1] - ia[0]
    return (a, b, oa ^ ob, ia[0], ia[1], ib[0], ib[1], n, n)


def _stored(genome_piece, o):
    return rc(genome_piece) if o else np.asarray(genome_piece, np.uint8).copy()


def linear(seed, n_reads=150, genome_len=6000, lo=300, hi=500, min_overlap=50, both_strands=True):
    """``n_reads`` reads of ``lo .. hi`` letters at random sorted positions of a random genome, the first pinned to its start and
    the last to its end, then permuted, on random strands.  Returns ``(genome, reads, records)`` with every true overlap of at
    least ``min_overlap`` letters."""
    rng = np.random.RandomState(seed)
    genome = rng.randint(0, 4, genome_len).astype(np.uint8)
    lens = rng.randint(lo, hi + 1, n_reads)
    starts = np.sort(rng.randint(0, genome_len - hi, n_reads))
    starts[0] = 0
    starts[-1] = genome_len - lens[-1]
    perm = rng.permutation(n_reads)                         # read perm[i] is the i-th along the genome
    orient = rng.randint(0, 2, n_reads) if both_strands else np.zeros(n_reads, int)
    reads = [None] * n_reads
    for i in range(n_reads):
        reads[perm[i]] = _stored(genome[starts[i]:starts[i] + lens[i]], orient[perm[i]])
    records = []
    for i in range(n_reads):
        for j in range(i + 1, n_reads):
            gs, ge = max(starts[i], starts[j]), min(starts[i] + lens[i], starts[j] + lens[j])
            if ge - gs < min_overlap:
                continue
            (x, y) = (i, j) if perm[i] < perm[j] else (j, i)
            a, b = int(perm[x]), int(perm[y])
            records.append(_record(a, b, int(orient[a]), int(orient[b]), int(lens[x]), int(lens[y]),
                                   (int(gs - starts[x]), int(ge - starts[x])), (int(gs - starts[y]), int(ge - starts[y]))))
    records.sort()
    return genome, reads, records


def ring(n=12, read_len=400, step=100, seed=1, both_strands=True):
    """A circular genome of ``n * step`` letters and ``n`` reads of ``read_len`` at every ``step``, in random order and on random
    strands; read ``i`` overlaps the ``d``-th read behind it while ``d * step < read_len``."""
    rng = np.random.RandomState(seed)
    G = n * step
    genome = rng.randint(0, 4, G).astype(np.uint8)
    perm = rng.permutation(n)
    orient = rng.randint(0, 2, n) if both_strands else np.zeros(n, int)
    reads = [None] * n
    for i in range(n):
        reads[perm[i]] = _stored(genome[(i * step + np.arange(read_len)) % G], orient[perm[i]])
    records = []
    for i in range(n):
        for d in range(1, n):
            if d * step >= read_len:
                break
            j = (i + d) % n
            assert (n - d) * step >= read_len, 'two overlaps of one pair'
            ii, ij = (d * step, read_len), (0, read_len - d * step)
            (x, y, ix, iy) = (i, j, ii, ij) if perm[i] < perm[j] else (j, i, ij, ii)
            a, b = int(perm[x]), int(perm[y])
            records.append(_record(a, b, int(orient[a]), int(orient[b]), read_len, read_len, ix, iy))
    records.sort()
    return genome, reads, records


def ladder(n=100, read_len=400, step=5, seed=1, both_strands=False, min_overlap=1):
    """``n`` reads of ``read_len`` at every ``step`` of a linear genome, in genome order: with 100 reads of 400 at step 5 a
    middle vertex has 79 arcs.  ``ladder(n, 100, 60)`` is a plain chain of ``n``: only neighbours overlap."""
    rng = np.random.RandomState(seed)
    genome = rng.randint(0, 4, (n - 1) * step + read_len).astype(np.uint8)
    orient = rng.randint(0, 2, n) if both_strands else np.zeros(n, int)
    reads = [_stored(genome[i * step:i * step + read_len], orient[i]) for i in range(n)]
    records = []
    for i in range(n):
        for j in range(i + 1, n):
            d = (j - i) * step
            if read_len - d < min_overlap:
                break
            records.append(_record(i, j, int(orient[i]), int(orient[j]), read_len, read_len, (d, read_len), (0, read_len - d)))
    return genome, reads, records


def is_rotation(x, y):
    x, y = bytes(bytearray(x)), bytes(bytearray(y))
    return len(x) == len(y) and x in y + y


def snapshot(G):
    """What a built ``OverlapGraph`` holds, in the shape of ``graph_ref.build``'s result: plain lists and tuples."""
    arcs, rows = G.arcs()
    unitigs, members = G.unitigs()
    return dict(cls=G.overlaps()['cls'].tolist(), contained=G.contained().tolist(), arcs=arcs.tolist(), rows=rows.tolist(),
                unitigs=unitigs[['first_member', 'length', 'n_members', 'head', 'circular']].tolist(), members=members.tolist())


def device_build(lens, records, **params):
    from biseqt_amd.graph import OverlapGraph
    with OverlapGraph(lens) as G:
        G.add(records)
        G.build(**params)
        return snapshot(G)
