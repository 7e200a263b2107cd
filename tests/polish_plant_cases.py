"""The planted pileup of tests/test_gpu_polish_reads.py, built without a device: a 300-column frame, four GLOBAL pairs over a
six-letter batch alphabet whose insertion runs fill the insertion plane of a four-letter pileup through ordinary adds (a
letter >= 4 lands in no slot: that is how a middle slot stays empty), and hand-made counts for every rule of the polish."""
import numpy as np

N_COLS, L, J = 300, 4, 3
# gaps cheaper than a substitution: the optimal GLOBAL alignment of a planted pair is its construction
GAPPY = dict(match_score=1, mismatch_score=-20, go_score=-2, ge_score=-1)
BIG = 2 ** 31 + 1


def frame():
    rng = np.random.default_rng(7801)
    f = rng.integers(0, L, N_COLS).astype(np.uint8)
    # no planted run can slide: its first letter differs from the frame letter behind it, its last from the one in front
    for col, (a, b) in {10: (2, 3), 20: (0, 1), 30: (0, 2), 33: (0, 2), 40: (0, 2), 45: (0, 1)}.items():
        f[col], f[col + 1] = a, b
    f[120:126] = 0
    return f


# inserted letters behind a column, per pair
_COMMON = {10: [0, 5, 1], 30: [1], 33: [1], 45: [2], 120: [1, 2, 3], 121: [1, 2, 3], 122: [1, 2, 3], 123: [1, 2, 3], 124: [1, 2, 3]}
PLANTS = [{**_COMMON, 20: [2], 40: [1]}, {**_COMMON, 20: [2], 40: [1]}, {**_COMMON, 20: [3]}, {20: [3]}]


def pairs():
    f = frame()
    out = []
    for plant in PLANTS:
        m = []
        for col, x in enumerate(f.tolist()):
            m.append(x)
            m.extend(plant.get(col, []))
        out.append((f.copy(), np.array(m, np.uint8)))
    return out


def expected_plane():
    """What the construction plants (the tests assert that the device's plane equals it)."""
    ins = np.zeros((N_COLS, J, L), np.uint32)
    for plant in PLANTS:
        for col, run in plant.items():
            for j, y in enumerate(run[:J]):
                if y < L:
                    ins[col, j, y] += 1
    return ins


def counts():
    """Random small counts (ties and empty columns abound), and the constructed columns."""
    rng = np.random.default_rng(7802)
    c = rng.integers(0, 4, size=(N_COLS, L + 2)).astype(np.uint32)
    c[10] = (1, 0, 3, 0, 0, 0)          # depth 4: slot 0 (3) passes, slot 1 (empty) fails, slot 2 (3) must not be emitted
    c[20] = (4, 0, 0, 0, 3, 0)          # depth 7, n_0 = 4: 8 > 7 passes; letters 2 and 3 tie: 2
    c[30] = (0, 0, 6, 0, 0, 0)          # depth 6, n_0 = 3: 6 > 6 fails
    c[33] = (0, 0, 5, 0, 0, 0)          # depth 5, n_0 = 3: 6 > 5 passes
    c[40] = (BIG, BIG, 0, 0, 0, 0)      # depth 2^32 + 2, n_0 = 2: passes only if compared in 32 bits
    c[45] = (1, 0, 0, 1, 0, 0)          # depth 2 < min_depth 3: the read's letter and no insertion; covered at min_depth 2
    c[46] = (0, 1, 2, 0, 0, 0)          # depth 3: on the other side of min_depth 3
    c[50] = (2 ** 32 - 1, 2, 0, 0, 0, 0)   # depth 2^32 + 1: below min_depth only in 32 bits
    c[60] = (2, 0, 0, 0, 2, 0)          # a letter ties with DEL: the letter
    c[61] = (0, 0, 0, 2, 2, 0)
    c[62] = (1, 2, 2, 0, 1, 0)          # two letters tie: the lower
    c[100:110] = (0, 1, 0, 0, 2, 0)     # a read whose every column is deleted
    c[120:125] = (3, 0, 0, 0, 0, 0)     # depth 3, every slot holds 3: 1 + J letters per column
    return c


def read_sets():
    """(offs, lens) per polish call: one read over frames of 1, 63, 64, 65 and 300 columns, the all-deleted read, the read that
    emits 1 + J letters per column, and 64, 65 and 1000 reads with lengths 0 among them."""
    sets = [([0], [n]) for n in (1, 63, 64, 65, 300)] + [([100], [10]), ([120], [5]), ([300], [0])]
    rng = np.random.default_rng(7803)
    for n in (64, 65, 1000):
        lens = rng.choice([0, 0, 1, 5, 63, 64, 65, 130], n)
        offs = np.array([rng.integers(0, N_COLS - ln + 1) for ln in lens])
        sets.append((offs.tolist(), lens.tolist()))
    return sets
