"""The oracle of the pileups (include/pw_pileup.h) in pure Python: one loop over the ops of a transcript that implements the
header's definition literally, and a numpy ``call`` of the columns.  No device code and no shared helper with the library."""
import numpy as np

ST_TRACED, ST_EMPTY, ST_PANICK, ST_BADPATH = 1, 2, 4, 8
COVERED, DIFFERS, INSERT = 1, 2, 4
SITE_DTYPE = np.dtype([('depth', '<u4'), ('call', 'u1'), ('ref', 'u1'), ('flags', '<u2')])


def contributes(status, transcript):
    """A pair adds to a pileup exactly when it would get a summary."""
    return bool(status & ST_TRACED) and not status & (ST_EMPTY | ST_PANICK | ST_BADPATH) and bool(transcript)


def add(counts, L, frame_start, origin_len, origin_idx, mutant_idx, transcript, mutant, status=ST_TRACED):
    """Add one pair to ``counts`` (``[n_cols, L + 2]``, in place).  ``frame_start`` is where the pair's origin frame starts
    in the pileup, ``mutant`` the letters of its mutant frame."""
    n_cols = len(counts)
    if not contributes(status, transcript):
        return
    if frame_start < 0 or frame_start + origin_len > n_cols:
        return
    c, q = frame_start + origin_idx, mutant_idx
    o = m = 0                                   # o(k), m(k)
    for k, op in enumerate(transcript):
        if op in 'MS':
            y = int(mutant[q + m])
            if y < L:
                counts[c + o, y] += 1
            o += 1
            m += 1
        elif op == 'D':
            counts[c + o, L] += 1
            o += 1
        elif op == 'I':
            if (k == 0 or transcript[k - 1] != 'I') and o > 0:
                counts[c + o - 1, L + 1] += 1
            m += 1


def zeros(n_cols, L):
    return np.zeros((n_cols, L + 2), np.uint32)


def of_batch(n_cols, L, res, txs, frames, mutants, origin_lens):
    """The pileup of one batch: ``res`` its records, ``txs`` its transcripts, ``frames[k]`` the frame start of pair k (None or
    negative: skipped), ``mutants[k]`` the letters of its mutant frame, ``origin_lens[k]`` the length of its origin frame."""
    counts = zeros(n_cols, L)
    for k, tx in enumerate(txs):
        if frames[k] is None:
            continue
        add(counts, L, int(frames[k]), int(origin_lens[k]), int(res['origin_idx'][k]), int(res['mutant_idx'][k]), tx, mutants[k],
            int(res['status'][k]))
    return counts


def call(counts, L, ref=None, min_depth=1):
    """One SITE_DTYPE record per column of ``counts`` (the rule of pw_pileup_call)."""
    counts = np.asarray(counts, np.uint32)
    n = len(counts)
    out = np.zeros(n, SITE_DTYPE)
    depth = counts[:, :L + 1].astype(np.uint64).sum(axis=1) & 0xffffffff
    covered = depth >= min_depth
    called = np.argmax(counts[:, :L + 1], axis=1) if n else np.zeros(0, np.int64)      # (argmax: the first of equal maxima)
    called = np.where(covered & (depth > 0), called, 255)
    out['depth'] = depth
    out['call'] = called
    out['ref'] = 255 if ref is None else np.asarray(ref, np.uint8)
    flags = np.where(covered, COVERED, 0)
    if ref is not None:
        flags = flags | np.where(covered & (called != np.asarray(ref, np.int64)), DIFFERS, 0)
    flags = flags | np.where(covered & (2 * counts[:, L + 1].astype(np.uint64) > depth), INSERT, 0)
    out['flags'] = flags
    return out
