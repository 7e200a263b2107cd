"""Fixtures of the consensus stage (include/pw_consensus.h), shared by tests/test_consensus_ref.py (CPU) and the GPU tests:
error-free read sets with planted containment chains, cycles and ties as records for tests/graph_ref.py, the noisy read set
of the whole-consensus experiment with its overlap records, and the oracle side of the consensus itself."""
import numpy as np

from tests import consensus_ref as CR
from tests import graph_cases as GC
from tests import graph_ref as GR
from tests import polish_cases as PC
from tests import polish_ref as PR

COMPLEMENT = GC.COMPLEMENT
CHAIN_LINKS = (1, 2, 3, 4, 5, 8, 9)
PARAMS = ((50, .1), (0, 0.), (7, .25))                 # (slack, drift) of the layouts the tests run


def chains(seed=3, links=CHAIN_LINKS, read_len=400, step=150):
    """An error-free backbone of reads of ``read_len`` at every ``step`` of a linear genome, on random strands and in random
    order, and on backbone read ``2 k + 1`` a chain of ``links[k]`` nested reads: each lies inside the one before and has a
    record with that one ALONE, so that its chain has exactly that many links.  Which of a pair has the lower index, and both
    strands, are random: every row of the header's table and both branches of the composition occur (the tests assert it).
    Returns ``(genome, reads, records, spans)``; ``spans[r] = (start, end, orientation)`` of read r on the genome."""
    rng = np.random.RandomState(seed)
    n_back = 2 * len(links) + 2
    genome = rng.randint(0, 4, (n_back - 1) * step + read_len).astype(np.uint8)
    spans = [(i * step, i * step + read_len) for i in range(n_back)]
    pairs = [(i, j) for i in range(n_back) for j in range(i + 1, n_back) if (j - i) * step < read_len]
    for k, n in enumerate(links):
        at = 2 * k + 1
        for _ in range(n):
            s, e = spans[at]
            spans.append((s + rng.randint(2, 20), e - rng.randint(2, 20)))
            pairs.append((at, len(spans) - 1))
            at = len(spans) - 1
    n = len(spans)
    perm = rng.permutation(n)                                # span i is read perm[i]
    orient = rng.randint(0, 2, n)                            # by read
    reads, where = [None] * n, [None] * n
    for i, (s, e) in enumerate(spans):
        reads[perm[i]] = GC._stored(genome[s:e], orient[perm[i]])
        where[perm[i]] = (s, e, int(orient[perm[i]]))
    records = []
    for i, j in pairs:
        (x, y) = (i, j) if perm[i] < perm[j] else (j, i)
        a, b = int(perm[x]), int(perm[y])
        gs, ge = max(spans[x][0], spans[y][0]), min(spans[x][1], spans[y][1])
        records.append(GC._record(a, b, int(orient[a]), int(orient[b]), spans[x][1] - spans[x][0], spans[y][1] - spans[y][0],
                                  (gs - spans[x][0], ge - spans[x][0]), (gs - spans[y][0], ge - spans[y][0])))
    records.sort()
    return genome, reads, records, where


def planted():
    """Small hand-planted graphs, ``{name: (reads, records)}``: the records need not come from a genome -- the device is compared
    with the oracle field by field.  Reads 0 .. 2 are a backbone of three dovetailed reads of 120, 100 and 110 letters."""
    rng = np.random.RandomState(11)

    def rd(n):
        return rng.randint(0, 4, n).astype(np.uint8)
    back = [(0, 1, 0, 60, 120, 0, 60, 60, 60), (1, 2, 1, 50, 100, 0, 50, 50, 50)]
    out = {}
    # a tie on n_match goes to the lowest record index (read 3: parents 0 and 1); a larger n_match at a higher index wins (read 4)
    out['tie'] = ([rd(120), rd(100), rd(110), rd(40), rd(40)],
                  back + [(3, 0, 0, 0, 40, 62, 102, 40, 40), (1, 3, 1, 2, 42, 0, 40, 40, 40),
                          (4, 0, 1, 0, 40, 70, 110, 38, 40), (4, 1, 0, 0, 40, 10, 50, 39, 40)])
    # mutually contained duplicates: a 2-cycle (3, 4), a 3-cycle (5, 6, 7), and read 8 that leads into the 2-cycle
    out['cycles'] = ([rd(120), rd(100), rd(110)] + [rd(80)] * 2 + [rd(70)] * 3 + [rd(30)],
                     back + [(3, 4, 0, 0, 80, 0, 80, 80, 80), (4, 3, 0, 0, 80, 0, 80, 80, 80),
                             (5, 6, 1, 0, 70, 0, 70, 70, 70), (6, 7, 0, 0, 70, 0, 70, 70, 70), (7, 5, 1, 0, 70, 0, 70, 70, 70),
                             (8, 3, 1, 0, 30, 20, 50, 30, 30)])
    # reads that stick out of their contig or miss it: on both end reads of the backbone, in both classes and strands, a child
    # whose alignment spans differ (negative pos with a task, or a clipped window) and one that only touches its parent's end
    # (pos + len == 0 or pos == the contig's length: no task); a zero-length read alone (7) and one that is contained (12)
    out['edges'] = ([rd(120), rd(100), rd(110), rd(100), rd(90), rd(50), rd(60), rd(0), rd(100), rd(90), rd(50), rd(60), rd(0)],
                    back + [(3, 0, 1, 0, 100, 60, 120, 60, 100), (4, 0, 1, 0, 90, 120, 120, 1, 90), (0, 5, 1, 0, 45, 0, 50, 45, 50),
                            (0, 6, 0, 0, 50, 0, 60, 50, 60),
                            (8, 2, 1, 0, 100, 60, 110, 50, 100), (9, 2, 1, 0, 90, 110, 110, 1, 90), (2, 10, 1, 0, 45, 0, 50, 45, 50),
                            (2, 11, 0, 60, 110, 10, 60, 50, 50), (12, 1, 0, 0, 0, 30, 60, 1, 30)])
    # no record at all: every read is a unitig of its own (a build without arcs)
    out['no_arcs'] = ([rd(37), rd(0), rd(64), rd(5)], [])
    return out


def infix_distance(contig, genome):
    """Unit-cost edit distance of the whole ``contig`` to the best stretch of ``genome``: the genome's two flanks are free."""
    a, b = np.asarray(contig, np.int64), np.asarray(genome, np.int64)
    idx = np.arange(len(b) + 1)
    prev = np.zeros(len(b) + 1, np.int64)
    for x in a:
        t = np.empty(len(b) + 1, np.int64)
        t[0] = prev[0] + 1
        t[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (b != x))
        prev = np.minimum.accumulate(t - idx) + idx
    return int(prev.min())


def errors(contigs, genome):
    """The contigs' error total: every contig against the genome or its reverse complement, whichever is nearer."""
    return sum(min(infix_distance(c, genome), infix_distance(c, PC.rc(genome))) for c in contigs)


# The whole-consensus experiment: the generator of tests/polish_cases.py (7 % errors: 3 % substitutions, 2 % insertions, 2 %
# deletions; reads of 400 letters on both strands) at about 25x over 2000 letters.
SEED, N_READS, GENOME = 7711, 125, 2000
SLACK, DRIFT = 50, .1
_cache = {}


def noisy_fixture():
    """dict(genome, fx): ``fx`` is ``polish_cases.fixture`` (reads, truth, pairs, strands, bands); the genome is drawn first by
    that generator, so the same seed gives it back (checked: every truth is a stretch of it or of its reverse complement)."""
    if 'fx' not in _cache:
        fx = PC.fixture(SEED, N_READS, GENOME)
        genome = np.random.Generator(np.random.PCG64(SEED)).integers(0, PC.L, GENOME, dtype=np.uint8)
        g, grc = genome.tobytes(), PC.rc(genome).tobytes()
        assert all(t.tobytes() in g or t.tobytes() in grc for t in fx['truth'])
        _cache['fx'] = dict(genome=genome, fx=fx)
    return _cache['fx']


def records_of(fx, alns):
    """Overlap records from alignments, as pw_batch_graph_add writes them: a pair without an alignment gives a NONE record."""
    out = []
    for (a, b), st, aln in zip(fx['pairs'], fx['strands'], alns):
        if aln is None or not aln['transcript']:
            out.append((a, b, int(st == '-'), 0, 0, 0, 0, 0, 0))
            continue
        t, oi, mi = aln['transcript'], aln['origin_start'], aln['mutant_start']
        n = {op: t.count(op) for op in 'MSID'}
        out.append((a, b, int(st == '-'), oi, oi + n['M'] + n['S'] + n['D'], mi, mi + n['M'] + n['S'] + n['I'], n['M'], len(t)))
    return out


def oracle_records(oracle):
    """The overlap records of the noisy fixture from CPU-oracle alignments of its truly overlapping pairs."""
    if 'records' not in _cache:
        fx = noisy_fixture()['fx']
        _cache['records'] = records_of(fx, PC.oracle_alignments(oracle, fx))
    return _cache['records']


def oracle_consensus(oracle, reads, records, slack=SLACK, drift=DRIFT, min_depth=PC.MIN_DEPTH, ins_slots=PC.INS_SLOTS,
                     self_weight=PC.SELF_WEIGHT, graph_params=None):
    """The whole stage on the oracle side, from overlap records to polished contigs: ``graph_ref.build`` and ``contigs``,
    ``consensus_ref`` for placements, tasks and the arena, CPU-oracle alignments of the tasks (banded B_OVERLAP 1 / -3 / -5 /
    -2), ``polish_ref`` for the pileup and the rule.  Returns a dict of everything on the way."""
    lens = [len(r) for r in reads]
    built = GR.build(lens, records, **(graph_params or {}))
    draft = [np.array(c, np.uint8) for c in GR.contigs(reads, built['unitigs'], built['members'], COMPLEMENT)]
    places = CR.place(lens, records, built)
    task_list, cstart, arena_bytes = CR.tasks(lens, places, built['unitigs'], slack, drift)
    arena = CR.arena(reads, draft, task_list, cstart, arena_bytes, COMPLEMENT)
    n_cols = cstart[-1]
    counts, ins = PR.zeros(n_cols, PC.L, ins_slots)
    PR.add_letters(counts, PC.L, arena[:n_cols], 0, self_weight)
    aligned = 0
    for col0, mut_off, r, win_len, dmin, dmax, _, _ in task_list:
        window, mutant = arena[col0:col0 + win_len], arena[mut_off:mut_off + lens[r]]
        res = oracle.solve(window, mutant, mode=oracle.BANDED_MODE, alntype=oracle.B_OVERLAP, L=PC.L, match=1, mismatch=-3, go=-5,
                           ge=-2, diag_range=(dmin, dmax))
        if not res.get('transcript'):
            continue
        aligned += 1
        PR.add(counts, ins, PC.L, col0, win_len, res['origin_idx'], res['mutant_idx'], res['transcript'], mutant)
    polished, stats = PR.polish(counts, ins, PC.L, arena, cstart[:-1], [u[1] for u in built['unitigs']], min_depth)
    return dict(built=built, draft=draft, places=places, tasks=task_list, cstart=cstart, arena=arena, aligned=aligned,
                contigs=[np.array(c, np.uint8) for c in polished], stats=stats)
