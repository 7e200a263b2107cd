"""The oracle of read correction (include/pw_polish.h) in pure Python: the origin-side add with insertion slots as one loop
over the ops of a transcript, ``swap`` and the reversed transformation written exactly as the header defines them, and
``polish`` with the per-read statistics.  No device code and no shared helper with the library."""
import numpy as np

ST_TRACED, ST_EMPTY, ST_PANICK, ST_BADPATH = 1, 2, 4, 8
STATS_DTYPE = np.dtype([(f, '<u4') for f in ('kept', 'substituted', 'deleted', 'inserted')])


def zeros(n_cols, L, J):
    """``(counts [n_cols, L + 2], ins [n_cols, J, L] or None for J == 0)``."""
    return np.zeros((n_cols, L + 2), np.uint32), (np.zeros((n_cols, J, L), np.uint32) if J else None)


def contributes(status, transcript):
    return bool(status & ST_TRACED) and not status & (ST_EMPTY | ST_PANICK | ST_BADPATH) and bool(transcript)


def add(counts, ins, L, frame_start, origin_len, origin_idx, mutant_idx, transcript, mutant, status=ST_TRACED):
    """THE primitive: add one pair to the columns of its origin.  ``counts`` and ``ins`` (or None) are changed in place,
    ``frame_start`` is where the origin frame starts in the pileup, ``mutant`` the letters of the mutant frame."""
    n_cols = len(counts)
    J = 0 if ins is None else ins.shape[1]
    if not contributes(status, transcript):
        return
    if frame_start < 0 or frame_start + origin_len > n_cols:
        return
    c, q = frame_start + origin_idx, mutant_idx
    o = m = 0                                   # o(k), m(k)
    run = 0                                     # 'I' ops directly in front of op k
    for op in transcript:
        if op == 'I':
            if o > 0:
                if run == 0:
                    counts[c + o - 1, L + 1] += 1
                if run < J:
                    y = int(mutant[q + m])
                    if y < L:
                        ins[c + o - 1, run, y] += 1
            run += 1
            m += 1
            continue
        run = 0
        if op in 'MS':
            y = int(mutant[q + m])
            if y < L:
                counts[c + o, y] += 1
            o += 1
            m += 1
        elif op == 'D':
            counts[c + o, L] += 1
            o += 1


def swap(transcript):
    return transcript.translate(str.maketrans('DI', 'ID'))


def add_mutant_side(counts, ins, L, frame_start, origin, mutant_len, origin_idx, mutant_idx, transcript, status=ST_TRACED):
    """The pair added to its MUTANT's columns: the origin-side add of the swapped pair.  ``origin``: the letters of the origin
    frame; ``frame_start``: where the mutant frame starts in the pileup."""
    if not transcript:
        return
    add(counts, ins, L, frame_start, mutant_len, mutant_idx, origin_idx, swap(transcript), origin, status)


def add_mutant_side_reversed(counts, ins, L, frame_start, origin, mutant_len, origin_idx, mutant_idx, transcript, complement,
                             status=ST_TRACED):
    """The mutant frame holds rc(read b), the columns are read b's forward letters: the origin-side add of
    (b, rc(origin frame), reverse(swap(t))) with the start indices of the header."""
    if not transcript:
        return
    X, Y = len(origin), mutant_len
    o_n = sum(transcript.count(op) for op in 'MSD')
    m_n = sum(transcript.count(op) for op in 'MSI')
    rc_origin = [int(complement[x]) if x < L else int(x) for x in list(origin)[::-1]]
    add(counts, ins, L, frame_start, Y, Y - (mutant_idx + m_n), X - (origin_idx + o_n), swap(transcript)[::-1], rc_origin, status)


def add_letters(counts, L, letters, lo, weight=1):
    for x, y in enumerate(letters):
        if int(y) < L:
            counts[lo + x, int(y)] += weight


def polish(counts, ins, L, letters, offs, lens, min_depth=1):
    """``(reads, stats)``: the polished reads as lists of letters, and one STATS_DTYPE record per read.  ``letters[c]`` is the
    letter of column c."""
    J = 0 if ins is None else ins.shape[1]
    reads, stats = [], np.zeros(len(offs), STATS_DTYPE)
    for r, (off, n) in enumerate(zip(offs, lens)):
        out = []
        kept = subst = deleted = inserted = 0
        for x in range(int(n)):
            col = int(off) + x
            s = int(letters[col])
            row = [int(v) for v in counts[col, :L + 1]]
            depth = sum(row)
            if depth < min_depth:
                out.append(s)
                kept += 1
                continue
            call = row.index(max(row))                       # (index: the first of equal maxima)
            if call == L:
                deleted += 1
            else:
                out.append(call)
                if call == s:
                    kept += 1
                else:
                    subst += 1
            for j in range(J):
                slot = [int(v) for v in ins[col, j]]
                if not 2 * sum(slot) > depth:
                    break
                out.append(slot.index(max(slot)))
                inserted += 1
        reads.append(out)
        stats[r] = (kept, subst, deleted, inserted)
    return reads, stats


def edit_distance(a, b):
    """Unit-cost global edit distance, a row at a time."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    idx = np.arange(len(b) + 1)
    prev = idx.copy()
    for x in a:
        t = np.empty(len(b) + 1, np.int64)
        t[0] = prev[0] + 1
        t[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (b != x))
        prev = np.minimum.accumulate(t - idx) + idx          # D[j] = min over k <= j of t[k] + (j - k)
    return int(prev[-1])
