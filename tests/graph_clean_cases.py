"""Planted layouts for the graph cleaning: reads are intervals on one coordinate axis, stored forwards or reverse-complemented,
and ONLY the pairs that a case joins get a record (tests/graph_cases.py's ``_record``) -- a spur or a side path is a read whose
other overlaps are simply not there, as with a read whose end is junk.  With reads of 100 letters and a step of 60 only
neighbours overlap, so nothing is reduced and every branch is what the case planted."""
import numpy as np

from tests import graph_cases as GC

L, STEP = 100, 60


class Layout(object):
    def __init__(self):
        self.start, self.length, self.orient, self.pairs, self.extra = [], [], [], [], []

    def read(self, start, orient=0, length=L):
        self.start.append(int(start)); self.length.append(int(length)); self.orient.append(int(orient))
        return len(self.start) - 1

    def join(self, *chain):
        """Records between consecutive reads of ``chain``."""
        for i, j in zip(chain, chain[1:]):
            self.pairs.append((i, j, self.start[j] - self.start[i]))

    def join_at(self, i, j, shift):
        """A record that puts read ``j`` ``shift`` letters behind read ``i``, whatever their coordinates say (a ring's closure)."""
        self.pairs.append((i, j, int(shift)))

    def line(self, n, start=0, step=STEP, orient=None):
        """``n`` reads at every ``step`` from ``start``, neighbours joined; ``orient``: one flag per read (default forwards)."""
        ids = [self.read(start + k * step, 0 if orient is None else orient[k]) for k in range(n)]
        self.join(*ids)
        return ids

    @property
    def lens(self):
        return list(self.length)

    def records(self):
        out = []
        for i, j, shift in self.pairs:
            a, b = min(i, j), max(i, j)
            sa, sb, la, lb = (0, shift, self.length[a], self.length[b]) if a == i else (shift, 0, self.length[a], self.length[b])
            gs, ge = max(sa, sb), min(sa + la, sb + lb)
            assert ge > gs, 'joined reads do not overlap'
            out.append(GC._record(a, b, self.orient[a], self.orient[b], la, lb, (gs - sa, ge - sa), (gs - sb, ge - sb)))
        return out + list(self.extra)                        # (records written out by the case itself)

    def reads(self, seed=5):
        """Random letters of the right lengths: contig letters are prefixes of reads, whatever the reads say."""
        rng = np.random.RandomState(seed)
        return [rng.randint(0, 4, n).astype(np.uint8) for n in self.length]


def spur(k, dead_end, at, flip=False, n_line=8):
    """A line of ``n_line`` reads and a spur of ``k`` reads: a dead start entering read ``at``, or a dead end leaving it.
    ``flip``: the spur's reads (and every second read of the line) are stored reverse-complemented.  Returns
    ``(layout, line ids, spur ids)``."""
    lay = Layout()
    line = lay.line(n_line, orient=[(i & 1) if flip else 0 for i in range(n_line)])
    sign = 1 if dead_end else -1
    ids = [lay.read(lay.start[at] + sign * (q + 1) * STEP, int(flip)) for q in range(k)]
    lay.join(at, *ids)
    return lay, line, ids


def fork(k1, k2):
    """A Y: two dead-start branches of ``k1`` and ``k2`` reads enter read 0 of a line of 6.  ``(layout, line, branch1, branch2)``."""
    lay = Layout()
    line = lay.line(6)
    b1 = [lay.read(-(q + 1) * STEP) for q in range(k1)]
    b2 = [lay.read(-(q + 1) * STEP) for q in range(k2)]
    lay.join(line[0], *b1)
    lay.join(line[0], *b2)
    return lay, line, b1, b2


def only_way_in():
    """A one-read path that is the only predecessor of a fork into two lines of 4: nothing competes with it."""
    lay = Layout()
    root = lay.read(0)
    up, down = lay.line(4, start=STEP), lay.line(4, start=STEP)
    lay.join(root, up[0])
    lay.join(root, down[0])
    return lay, root, up, down


def bubble(sizes, tail=3, circular=False, orient=0):
    """A source line of ``tail`` reads, ``len(sizes)`` parallel paths of ``sizes[q]`` reads between its last read and the first
    read of a sink line of ``tail`` reads.  Path q's reads lie evenly between source and sink.  ``circular``: the sink line's
    last read is joined back to the source line's first, as if the genome were a ring.  ``(layout, source, paths, sink)``."""
    lay = Layout()
    src = lay.line(tail, orient=[orient] * tail)
    s0 = lay.start[src[-1]]
    gap = 2 * STEP                                           # source's last read to the sink's first: too far to overlap
    paths = []
    for n in sizes:
        ids = [lay.read(s0 + (q + 1) * gap // (n + 1), orient) for q in range(n)]
        paths.append(ids)
    snk = lay.line(tail, start=s0 + gap, orient=[orient] * tail)
    for ids in paths:
        lay.join(src[-1], *(ids + [snk[0]]))
    if circular:
        lay.join_at(snk[-1], src[0], STEP)                   # the ring closes
    return lay, src, paths, snk


def spur_on_bubble():
    """A 1-against-2 bubble whose two-read path carries a one-read dead-end spur on its first read: the spur splits that path,
    so the first round sees no parallel candidate and only drops the spur; the second round pops the bubble.
    ``(layout, spur ids, short path, long path)``."""
    lay, _, (short, long_), _ = bubble((1, 2))
    x = lay.read(lay.start[long_[0]] + STEP)
    lay.join(long_[0], x)
    return lay, [x], short, long_


def different_sinks():
    """Two paths of one and two reads leave one source for two different sink lines: no bubble.  ``(layout, paths)``."""
    lay = Layout()
    src = lay.line(3)
    s0 = lay.start[src[-1]]
    a = [lay.read(s0 + STEP)]
    b = [lay.read(s0 + 40), lay.read(s0 + 80)]
    sink_a, sink_b = lay.line(3, start=s0 + 2 * STEP), lay.line(3, start=s0 + 2 * STEP)
    lay.join(src[-1], *(a + [sink_a[0]]))
    lay.join(src[-1], *(b + [sink_b[0]]))
    return lay, [a, b]


def hairpin(second_path=True):
    """A line of 3 ends in read s; path x (one read) leaves s and comes back to the reverse complement of s, so {x} and its
    twin are two parallel candidates from s to s ^ 1 with equal n and mr: neither goes.  ``second_path``: reads y1, y2 run
    the same way round, and x loses against them.  ``(layout, s, x, [y1, y2])``."""
    lay = Layout()
    line = lay.line(3)
    s = line[-1]
    x = lay.read(lay.start[s] + STEP)
    lay.join(s, x)
    lay.extra.append((s, x, 1, STEP, L, 0, L - STEP, L - STEP, L - STEP))          # s+ -> x-, and its twin x+ -> s-
    ys = []
    if second_path:
        ys = [lay.read(lay.start[s] + 40), lay.read(lay.start[s] + 80)]
        lay.join(s, *ys)
        lay.extra.append((s, ys[1], 1, 40, L, 0, L - 40, L - 40, L - 40))          # s+ -> y2-, and its twin y2+ -> s-
    return lay, s, x, ys


def comb(n=140, every=10, fan_at=70, fan=70):
    """A line of ``n`` reads (2n vertices: more than one workgroup) with a one-read spur at every ``every``-th read, dead
    ends and dead starts in turn and on either strand, ``fan`` dead ends on read ``fan_at`` alone -- a row of more than 64
    arcs -- and an isolated component of two reads.  ``(layout, spur ids, isolated ids)``."""
    lay = Layout()
    line = lay.line(n, orient=[(i // 3) & 1 for i in range(n)])
    spurs = []
    for q, at in enumerate(range(every, n, every)):
        sign = 1 if q & 1 else -1
        x = lay.read(lay.start[line[at]] + sign * STEP, q & 2 and 1)
        lay.join(line[at], x)
        spurs.append(x)
    for q in range(fan):
        x = lay.read(lay.start[line[fan_at]] + 30 + (q % 50), q & 1)
        lay.join(line[fan_at], x)
        spurs.append(x)
    iso = lay.line(2, start=10 ** 6)
    return lay, spurs, iso


def hanging():
    """For the placements: a line of 6; a two-read dead end x1, x2 on read 2 (x2 overlaps nothing that stays); a read c of 50
    letters contained in x1.  ``(layout, x1, x2, c)``."""
    lay = Layout()
    line = lay.line(6, orient=[0, 1, 0, 0, 1, 0])
    x1 = lay.read(lay.start[line[2]] + STEP, 1)
    x2 = lay.read(lay.start[line[2]] + 2 * STEP)
    lay.join(line[2], x1, x2)
    c = lay.read(lay.start[x1] + 20, 0, length=50)
    lay.join(x1, c)
    return lay, x1, x2, c


def junk_tails(seed=11, genome_len=3000, read_len=400, stride=100, at=((250, 0), (1450, 1))):
    """Raw reads for ``assemble_reads``: a random genome tiled by error-free reads of ``read_len`` at every ``stride``, stored
    forwards and reverse-complemented in turn, plus one read per ``(position, strand)`` of ``at`` -- a stretch of the genome off
    the tiling's grid, stored on that strand, whose last third AS STORED is random letters.  Such a read overlaps cleanly with
    the reads before its good end and with nothing after its junk: a one-read dead end (or dead start) on the line.
    Returns ``(genome, reads, ids of the planted reads, (start, orientation) per read)``."""
    rng = np.random.RandomState(seed)
    genome = rng.randint(0, 4, genome_len).astype(np.uint8)
    where = [(s, (s // stride) & 1) for s in range(0, genome_len - read_len + 1, stride)]
    reads = [GC._stored(genome[s:s + read_len], o) for s, o in where]
    planted = []
    for s, o in at:
        r = GC._stored(genome[s:s + read_len], o)
        r[read_len - read_len // 3:] = rng.randint(0, 4, read_len // 3)
        planted.append(len(reads))
        reads.append(r)
        where.append((s, o))
    return genome, reads, planted, where
