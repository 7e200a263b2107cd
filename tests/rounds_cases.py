"""Fixtures of the iterated consensus (include/pw_rounds.h), shared by tests/test_rounds_ref.py (CPU) and the GPU tests: the
read sets of tests/polish_plant_cases.py in the shape the column polish accepts, a wide pileup whose reads straddle the
256-column chunks of the device's grid, and hand-made polished sets for the relayout."""
import numpy as np

from tests import polish_plant_cases as PP


def _disjoint(offs, lens):
    """The reads of a set in column order with every overlap cut away (a read keeps what lies behind the one before)."""
    out_o, out_n, end = [], [], 0
    for off, n in sorted(zip(offs, lens)):
        lo = max(off, end)
        hi = max(off + n, lo)
        out_o.append(lo); out_n.append(hi - lo)
        end = hi
    return out_o, out_n


def ordered_read_sets():
    """``polish_plant_cases.read_sets()`` in column order and without overlaps: the single reads are unchanged; the random
    sets of 64, 65 and 1000 reads are sorted and clipped, zero lengths among them."""
    return [_disjoint(offs, lens) for offs, lens in PP.read_sets()]


# ---- the wide pileup: 1100 columns, L = 4, J = 8 ----
WIDE_COLS, WIDE_L, WIDE_J = 1100, 4, 8
# reads of 255, 256 and 257 columns separated by gaps of 0, 1 and 3 columns behind an unread head of 5 columns; then either a
# read of 255 columns and an unread tail, or a read that ends at n_cols (and takes two chunks of the grid)
WIDE_HEAD = ([5, 260, 517, 777], [255, 256, 257])
WIDE_READ_SETS = [(WIDE_HEAD[0], WIDE_HEAD[1] + [255]), (WIDE_HEAD[0], WIDE_HEAD[1] + [WIDE_COLS - 777]),
                  ([0], [WIDE_COLS]), ([0, 256, 512, 768, 1024], [256, 256, 256, 256, 76]), ([1099], [1])]
# inserted letters behind a column: runs of 1 .. 10 letters at the edges of the chunks and of the reads
WIDE_PLANTS = [{4: [1], 5: [2, 3], 259: [0, 1, 2], 260: [3] * 4, 300: [0, 1, 2, 3, 0, 1, 2, 3], 301: [1] * 10, 515: [2] * 5, 516: [0],
                517: [1, 2], 700: [3, 2, 1, 0, 3, 2, 1, 0, 3], 773: [2] * 8, 776: [1], 777: [0] * 6, 1031: [3] * 7, 1032: [1], 1098: [2, 2]},
               {5: [2, 3], 260: [3] * 4, 300: [0, 1, 2, 3, 0, 1, 2, 3], 516: [0], 700: [3, 2, 1], 777: [0] * 6, 1098: [2]}]


def wide_frame():
    rng = np.random.default_rng(7830)
    return rng.integers(0, WIDE_L, WIDE_COLS).astype(np.uint8)


def wide_pairs():
    """(frame, frame with the planted runs) per plant: GLOBAL alignments with gaps cheaper than a substitution put every run
    behind its column, or behind a neighbour where the letters let it slide -- the tests read the plane back and compare
    with the oracle on exactly that plane."""
    f = wide_frame()
    out = []
    for plant in WIDE_PLANTS:
        m = []
        for col, x in enumerate(f.tolist()):
            m.append(x)
            m.extend(plant.get(col, []))
        out.append((f.copy(), np.array(m, np.uint8)))
    return out


def wide_counts(ins):
    """Counts for the plane ``ins`` as the device holds it: depths of 0 .. 3 (so that a slot that one or two pairs filled
    passes here and fails there), a deletion here and there, and depth 1 on a letter wherever all eight slots are filled:
    those columns emit nine letters."""
    rng = np.random.default_rng(7831)
    c = np.zeros((WIDE_COLS, WIDE_L + 2), np.uint32)
    ch = rng.integers(0, WIDE_L + 1, WIDE_COLS)
    c[np.arange(WIDE_COLS), ch] = rng.integers(0, 4, WIDE_COLS)
    nine = np.flatnonzero((ins.sum(2) >= 1).all(1))
    c[nine] = 0
    c[nine, 2] = 1
    return c, nine


# ---- hand-made polished sets for the relayout ----
VARIANTS = ('identity', 'ends deleted', 'nine', 'first contig empty', 'grow by one', 'grow by four', 'random')


def emitted(variant, lengths, seed=0):
    """``e`` per contig: how many letters every column of the layout's contigs emits in the hand-made set ``variant``."""
    rng = np.random.default_rng(7840 + seed)
    out = []
    for u, n in enumerate(lengths):
        e = np.ones(int(n), np.int64)
        if variant == 'ends deleted' and n:
            e[0] = e[-1] = 0
        elif variant == 'nine' and n:
            e[min(1, n - 1)] = 9
        elif variant == 'first contig empty' and u == 0:
            e[:] = 0
        elif variant == 'grow by one' and n:
            e[0] = 2                     # 37 -> 38 letters stays below the next 4-byte boundary, 40 -> 41 crosses it
        elif variant == 'grow by four' and n:
            e[n // 2] = 5                # every later cstart moves by 4
        elif variant == 'random':
            e = rng.choice([0, 1, 1, 1, 1, 2, 3], int(n)).astype(np.int64)
        out.append(e)
    return out


def polished_set(variant, draft, lengths, cstart, seed=0):
    """``(polished contigs, letters, offsets uint64[n_unitigs + 1], colmap uint64[n_cols + 1])`` of the hand-made set: a
    column that emits one letter emits the draft's, every other emitted letter is random."""
    rng = np.random.default_rng(7850 + seed)
    n_cols = int(cstart[-1])
    e_all = np.zeros(n_cols + 1, np.int64)
    contigs = []
    for u, e in enumerate(emitted(variant, lengths, seed)):
        e_all[cstart[u]:cstart[u] + len(e)] = e
        d = np.asarray(draft[u], np.uint8)
        out = []
        for x, k in enumerate(e.tolist()):
            out.extend([int(d[x])] if k == 1 else rng.integers(0, 4, k).tolist())
        contigs.append(np.array(out, np.uint8))
    colmap = np.concatenate([[0], np.cumsum(e_all[:-1])]).astype(np.uint64)
    offsets = np.array([colmap[cstart[u]] for u in range(len(lengths))] + [colmap[n_cols]], np.uint64)
    letters = np.concatenate(contigs) if contigs else np.zeros(0, np.uint8)
    return contigs, letters.astype(np.uint8), offsets, colmap
