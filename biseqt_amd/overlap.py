"""Overlap discovery for many read pairs: band selection in one GPU pass, then one banded overlap-alignment batch.

The reference scores every pair of reads with its own ``WordBlotOverlap`` object
(``experiments/blot_overlaps.py:262-272``, ``biseqt/blot.py:497-579``).  :func:`overlap_bands` returns, per pair, the
same dict ``highest_scoring_overlap_band()`` returns (``d_band``, ``p``, ``len``, ``score``; None without seeds), all
pairs scored by one call into ``include/pw_overlap.h``; :func:`overlap_alignments` then gives every band to the
banded overlap aligner (``B_OVERLAP``) in one batch -- BASELINE config 4's "seeding -> banded DP".
Pairs for which more than one diagonal could reach the same estimated match probability (where the reference's
answer depends on the order of its seeds table) are re-scored by the single-pair path, which reproduces that order.
One documented divergence: two reads with IDENTICAL content are scored here as two different sequences, whereas the
reference turns such a pair into a self comparison (``seeds.py:33``) and ignores its main diagonal.

Both strands: reads come from either strand of the molecule, so every entry point takes strands.  A minus-strand pair
``(a, b, '-')`` is the pair ``S = reads[a]``, ``T = rc(reads[b])``; diagonals, bands, start indices and transcripts are
in the frame of that ``T`` (position ``j'`` of ``T`` is letter ``len(b) - 1 - j'`` of ``reads[b]``, complemented) and
equal what the forward code returns for ``(a, rc(b))`` with ``rc(b)`` materialised.  :func:`minus_to_forward` maps a
result back to forward coordinates of ``reads[b]``.  A read is never paired with its own reverse complement.

Minimizer sampling (``minimizer_window`` of the all-pairs calls): the index holds only the window minimizers of every read
(``include/pw_kmers.h`` states the rule), so the sort, the join and the seed sort shrink by the density, about
``2 / (window + 1)``.  A seed then exists only between two selected k-mers.  What this means for a caller:

* ``p`` of a sampled band is the estimate from the SAMPLED seeds: it lies below the unsampled one (a true overlap keeps about
  the density's share of its seeds, and ``p`` is the ``wordlen``-th root of the seed excess per letter);
* a ``p_min`` threshold of :func:`overlap_alignments` therefore needs rescaling by the caller -- ``stats['density']`` is there
  for that;
* ``d_band`` (``d_best`` / ``r_best`` of the record), which the alignment stage consumes, is unaffected in kind: the best
  diagonal of the surviving seeds and the radius of its overlap length.
"""
import ctypes as C

import numpy as np
from scipy.special import erfcinv

from . import _pwlib as W
from .batch import BatchAligner
from .blot import H1_moments, WordBlotOverlap
from .kmers import check_window
from .sequence import Alphabet, Sequence, check_complement, complement_table, reverse_complement

BAND_DTYPE = np.dtype([('n_seeds', '<i8'), ('w_best', '<f8'), ('d_best', '<i4'), ('n_best', '<i4'),
                       ('r_best', '<i4'), ('len_best', '<i4'), ('band_best', '<i4'), ('tie', '<i4'),
                       ('d_first', '<i4'), ('n_first', '<i4'), ('r_first', '<i4'), ('len_first', '<i4'),
                       ('band_first', '<i4'), ('pad_', '<i4')])
assert BAND_DTYPE.itemsize == 64


def _arena(reads):
    arrs = [r.as_array(np.uint8) if isinstance(r, Sequence) else np.ascontiguousarray(r, np.uint8) for r in reads]
    offs = np.zeros(len(arrs) + 1, np.int64)
    offs[1:] = np.cumsum([len(a) for a in arrs])
    arena = np.concatenate(arrs) if arrs else np.zeros(0, np.uint8)
    return arena, offs, arrs


def _same(a, b):
    a = a.as_array(np.uint8) if isinstance(a, Sequence) else np.asarray(a)
    b = b.as_array(np.uint8) if isinstance(b, Sequence) else np.asarray(b)
    return len(a) == len(b) and bool((a == b).all())


_STRAND_SEL = {'+': W.PW_STRAND_PLUS, '-': W.PW_STRAND_MINUS, 'both': W.PW_STRAND_BOTH}


def _strand_flags(strands, n):
    """A per-pair strand list (``'+'`` / ``'-'``, or 0 / 1) as a uint8 array of 0 (+) and 1 (-); None stays None."""
    if strands is None:
        return None
    flags = np.zeros(n, np.uint8)
    strands = list(strands)
    if len(strands) != n:
        raise ValueError('one strand per pair: %d strands for %d pairs' % (len(strands), n))
    for q, st in enumerate(strands):
        if isinstance(st, str) and st in ('+', '-'):
            flags[q] = st == '-'
        elif not isinstance(st, str) and st in (0, 1):
            flags[q] = st
        else:
            raise ValueError("a strand is '+' or '-' (or 0 / 1), not %r" % (st,))
    return flags


def _complement(complement, alphabet_len, alphabet=None):
    """The complement table of a call: a table of ``alphabet_len`` letter indices or, with an :class:`Alphabet`, the
    ``mappings`` of ``Alphabet.transform``."""
    if complement is None:
        raise ValueError("minus-strand pairs need a complement, e.g. complement_table(Alphabet('ACGT'), [('A', 'T'), ('C', 'G')])")
    if alphabet is not None and (isinstance(complement, dict) or
                                 (isinstance(complement, list) and complement and isinstance(complement[0], (tuple, list)))):
        return complement_table(alphabet, complement)
    return check_complement(complement, alphabet_len)


def minus_to_forward(mutant_start, transcript, mutant_len):
    """An alignment of a minus-strand pair in forward coordinates of ``reads[b]``: the transcript covers positions
    ``[mutant_start, mutant_end)`` of ``T = rc(reads[b])`` (``M``, ``S`` and ``I`` consume a letter of ``T``), which are the
    letters ``[len(b) - mutant_end, len(b) - mutant_start)`` of ``reads[b]``, read backwards and complemented.  Returns
    that half-open forward interval ``(start, end)``."""
    tx = transcript.encode('ascii') if isinstance(transcript, str) else bytes(transcript)
    mutant_end = mutant_start + sum(tx.count(op) for op in b'MSI')
    assert 0 <= mutant_start <= mutant_end <= mutant_len
    return mutant_len - mutant_end, mutant_len - mutant_start


def reverse_strand_keys(read, wordlen, alphabet_len, complement):
    """Host restatement of the device's reverse-strand encoder: the k-mer keys of ``rc(read)`` at every position ``j'``,
    computed from the FORWARD letters -- key(j') = sum over t of complement[read[len - 1 - j' - t]] * L^(k - 1 - t) -- without
    materialising ``rc(read)``.  It is the forward key of the materialised reverse complement at ``j'``, and the reverse
    complement (digits reversed and complemented) of the forward key of ``read`` at ``len - k - j'``."""
    read = np.asarray(read, np.int64)
    comp = check_complement(complement, alphabet_len).astype(np.uint64)
    n = len(read) - wordlen + 1
    if n <= 0:
        return np.zeros(0, np.uint64)
    idx = (len(read) - 1 - np.arange(n))[:, None] - np.arange(wordlen)[None, :]
    weights = np.uint64(alphabet_len) ** np.arange(wordlen - 1, -1, -1, dtype=np.uint64)
    return (comp[read[idx]] * weights[None, :]).sum(axis=1, dtype=np.uint64)


def _band_coeffs(g_max, sensitivity, alphabet_len, wordlen):
    """``(len_coeff, radius_coeff, word_p_null)`` of the C calls: the reference's constants, computed as it computes them
    (blot.py:109, 134-136, 538) -- they reach the device as doubles."""
    len_coeff = 2. / (2 - g_max)
    radius_coeff = erfcinv(1. - sensitivity) * np.sqrt(2 * g_max)
    word_p_null = (1. / alphabet_len) ** wordlen
    return float(len_coeff), float(radius_coeff), float(word_p_null)


def raw_bands(reads, pairs, wordlen, alphabet_len, g_max, sensitivity, device=0, strands=None, complement=None):
    """The device records (BAND_DTYPE) for ``pairs`` = list of (i, j) indices into ``reads``; also returns the
    device time in ms.  ``strands``: one ``'+'`` / ``'-'`` per pair (default: all ``'+'``); a minus pair is scored against
    the reverse complement of ``reads[j]`` under the table ``complement``."""
    assert 0 < g_max < 1 and 0 < sensitivity < 1
    flags = _strand_flags(strands, len(pairs))
    comp = _complement(complement, alphabet_len) if flags is not None and flags.any() else None
    lib = W.load()
    arena, offs, arrs = _arena(reads)
    n = len(pairs)
    rp = (W.pw_read_pair * max(n, 1))()
    for q, (i, j) in enumerate(pairs):
        rp[q] = W.pw_read_pair(int(offs[i]), int(offs[j]), len(arrs[i]), len(arrs[j]))
    out = np.zeros(max(n, 1), BAND_DTYPE)
    coeffs = _band_coeffs(g_max, sensitivity, alphabet_len, wordlen)
    arena_c = np.ascontiguousarray(arena)
    if comp is None:
        name = 'pw_overlap_bands'
        rc = lib.pw_overlap_bands(device, arena_c.ctypes.data, arena_c.size, rp, n, alphabet_len, wordlen, *coeffs, out.ctypes.data)
    else:
        name = 'pw_overlap_bands_stranded'
        rc = lib.pw_overlap_bands_stranded(device, arena_c.ctypes.data, arena_c.size, rp, n, alphabet_len, wordlen, *coeffs,
                                           comp.ctypes.data, flags.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise RuntimeError(name + ' failed: ' + (lib.pw_overlap_last_error() or b'').decode())
    return out[:n], lib.pw_overlap_last_ms()


def _result(d, rad, L, n_in_band, word_p, alphabet_len, wordlen):
    if not word_p > 0:                                   # blot.py:541-545
        p_hat = 0
    else:
        p_hat = np.exp(np.log(word_p) / wordlen)
    p_hat = min(p_hat, 1)
    rad = np.float64(rad)                                # the reference carries np.ceil's float
    res = {'d_band': (d - rad, d + rad), 'p': p_hat, 'len': int(L)}
    area = 2 * rad * L
    mu_H1, sd_H1 = H1_moments(alphabet_len, wordlen, area, L, p_hat)
    res['score'] = (n_in_band - mu_H1) / sd_H1
    return res


def _records_to_results(reads, pairs, recs, wordlen, alphabet, g_max, sensitivity, device, flags=None, comp=None, fallback=True):
    """Device records -> the reference's dicts (shared by the pair-list and the all-pairs paths).  ``flags``: 0 / 1 per pair
    (None: all forward); the T of a minus pair is the reverse complement of its read.  ``fallback=False``: a ``tie > 1`` pair
    keeps the record's own choice (largest ``w``, then smallest ``d``) instead of going to the single-pair path."""
    L = len(alphabet)
    out, n_fallback = [], 0

    def t_of(q):
        T = reads[pairs[q][1]]
        return reverse_complement(T, comp) if flags is not None and flags[q] else T

    for q, r in enumerate(recs):
        if r['n_seeds'] == 0:
            out.append(None)
        elif not r['w_best'] > 0:
            # every p is 0: max() keeps the first row of the table (blot.py:569)
            word_p = (r['n_first'] + 1 - (2 * int(r['r_first']) * int(r['len_first'])) * ((1. / L) ** wordlen)) / r['len_first']
            out.append(_result(int(r['d_first']), int(r['r_first']), int(r['len_first']), int(r['band_first']), word_p, L, wordlen))
        elif fallback and r['tie'] > 1 and not _same(reads[pairs[q][0]], t_of(q)):
            i, T = pairs[q][0], t_of(q)
            S = reads[i] if isinstance(reads[i], Sequence) else Sequence(alphabet, tuple(int(c) for c in reads[i]))
            T = T if isinstance(T, Sequence) else Sequence(alphabet, tuple(int(c) for c in T))
            wb = WordBlotOverlap(S, T, g_max=g_max, sensitivity=sensitivity, alphabet=alphabet, wordlen=wordlen, device=device)
            out.append(wb.highest_scoring_overlap_band())
            wb.close()
            n_fallback += 1
        else:
            out.append(_result(int(r['d_best']), int(r['r_best']), int(r['len_best']), int(r['band_best']), float(r['w_best']), L, wordlen))
    return out, n_fallback


def overlap_bands(reads, pairs, wordlen, alphabet, g_max, sensitivity, device=0, stats=None, strands=None, complement=None):
    """``highest_scoring_overlap_band()`` of every pair ``(i, j)`` (``reads[i]`` as S, ``reads[j]`` as T -- or, where
    ``strands[q]`` is ``'-'``, the reverse complement of ``reads[j]`` as T).  ``complement``: a table or the ``mappings`` of
    ``Alphabet.transform``, e.g. ``[('A', 'T'), ('C', 'G')]``."""
    assert isinstance(alphabet, Alphabet)
    flags = _strand_flags(strands, len(pairs))
    comp = _complement(complement, len(alphabet), alphabet) if flags is not None and flags.any() else None
    recs, ms = raw_bands(reads, pairs, wordlen, len(alphabet), g_max, sensitivity, device, strands=flags, complement=comp)
    out, n_fallback = _records_to_results(reads, pairs, recs, wordlen, alphabet, g_max, sensitivity, device, flags, comp)
    if stats is not None:
        stats.update(device_ms=ms, fallback_pairs=n_fallback, pairs=len(pairs))
    return out


def raw_all_pairs(reads, wordlen, alphabet_len, g_max, sensitivity, device=0, max_pairs=None, rank=0, world=1, strands='+',
                  complement=None, with_strand=None, max_kmer_occ=None, stats=None, minimizer_window=None):
    """All pairs ``a < b`` of ``reads`` that share at least one seed, through ONE k-mer index over all reads:
    returns ``(pairs (n, 2) int32, records BAND_DTYPE, device ms)``.  With ``world > 1`` only the pairs whose smaller
    read index is ``rank`` modulo ``world`` (one process per GPU, no data-path collective).

    ``strands``: ``'+'`` (read a against read b, the default), ``'-'`` (read a against the reverse complement of read b
    under the table ``complement``) or ``'both'``.  With ``with_strand`` (default: whenever ``strands`` is not ``'+'``) the
    call goes through ``pw_overlap_all_pairs_stranded`` and returns ``(pairs, strand (n,) uint8: 0 '+' / 1 '-', records,
    device ms)``, in ascending ``(a, b, strand)`` order.

    ``max_kmer_occ``: None or 0 (today's calls, unchanged), or the occurrence cap of ``pw_overlap_all_pairs_capped``: a k-mer
    that occurs more than ``max_kmer_occ`` times in the whole read set (both strands counted unless ``strands == '+'``) gives
    no seeds.  ``stats`` (a dict) then receives the fields of ``pw_overlap_cap_stats``: ``entries``, ``masked_entries``,
    ``distinct_masked``, ``seeds_kept``, ``seeds_dropped``.

    ``minimizer_window``: None, 0 or 1 (today's calls, unchanged), or a window of 2..128: the call goes through
    ``pw_overlap_all_pairs_sampled`` and only the window minimizers of every read are indexed -- under the plain order of a
    k-mer's mixed key with ``strands='+'``, under the canonical order (the smaller of the k-mer and its reverse complement)
    otherwise.  Every record is the documented record of the seeds between two selected k-mers; ``w_best`` (and the ``p``
    made of it) is the estimate from those seeds and lies below the unsampled one, ``d_best`` / ``r_best`` are unaffected in
    kind.  The cap then counts occurrences in the sampled index.  ``stats`` receives ``positions`` (forward k-mer positions),
    ``sampled`` (those indexed) and ``density`` (their ratio).  Anything but None or an integer in 0..128 is a ValueError."""
    assert 0 < g_max < 1 and 0 < sensitivity < 1
    window = check_window(minimizer_window, 'minimizer_window')
    if max_kmer_occ is not None and not 0 <= int(max_kmer_occ) < 2 ** 32:
        raise ValueError('max_kmer_occ is None or 0 (no cap) or a count below 2^32, not %r' % (max_kmer_occ,))
    if strands not in _STRAND_SEL:
        raise ValueError("strands is '+', '-' or 'both', not %r" % (strands,))
    if with_strand is None:
        with_strand = strands != '+'
    if strands != '+' and not with_strand:
        raise ValueError('minus-strand pairs come with their strand column')
    comp = _complement(complement, alphabet_len) if strands != '+' else None
    lib = W.load()
    arena, offs, arrs = _arena(reads)
    R = len(arrs)
    cap = int(max_pairs) if max_pairs is not None else min(R * (R - 1) // 2 * (2 if strands == 'both' else 1), 1 << 26)
    pa, pb = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32)
    out = np.zeros(max(cap, 1), BAND_DTYPE)
    n_out = C.c_int64(0)
    roff = np.ascontiguousarray(offs[:-1].astype(np.uint64))
    rlen = np.ascontiguousarray(np.diff(offs).astype(np.int32))
    arena_c = np.ascontiguousarray(arena)
    coeffs = _band_coeffs(g_max, sensitivity, alphabet_len, wordlen)
    if window > 1:
        ps = np.zeros(max(cap, 1), np.uint8)
        cs, ss = W.pw_overlap_cap_stats(), W.pw_overlap_sample_stats()
        rc = lib.pw_overlap_all_pairs_sampled(device, arena_c.ctypes.data, arena_c.size, roff.ctypes.data, rlen.ctypes.data, R,
                                              alphabet_len, wordlen, *coeffs, None if comp is None else comp.ctypes.data,
                                              _STRAND_SEL[strands], int(rank), int(world), cap, pa.ctypes.data, pb.ctypes.data,
                                              ps.ctypes.data, out.ctypes.data, C.byref(n_out), int(max_kmer_occ or 0), C.byref(cs),
                                              window, C.byref(ss))
        if stats is not None:
            if max_kmer_occ:
                stats.update((f, int(getattr(cs, f))) for f, _ in cs._fields_)
            stats.update(positions=int(ss.positions), sampled=int(ss.sampled),
                         density=float(ss.sampled) / ss.positions if ss.positions else float('nan'))
        if rc != 0:
            raise RuntimeError('pw_overlap_all_pairs_sampled failed: ' + (lib.pw_overlap_last_error() or b'').decode())
        n = n_out.value
        pairs = np.stack([pa[:n], pb[:n]], axis=1)
        return (pairs, ps[:n], out[:n], lib.pw_overlap_last_ms()) if with_strand else (pairs, out[:n], lib.pw_overlap_last_ms())
    if max_kmer_occ:
        ps = np.zeros(max(cap, 1), np.uint8)
        cs = W.pw_overlap_cap_stats()
        rc = lib.pw_overlap_all_pairs_capped(device, arena_c.ctypes.data, arena_c.size, roff.ctypes.data, rlen.ctypes.data, R,
                                             alphabet_len, wordlen, *coeffs, None if comp is None else comp.ctypes.data,
                                             _STRAND_SEL[strands], int(rank), int(world), cap, pa.ctypes.data, pb.ctypes.data,
                                             ps.ctypes.data, out.ctypes.data, C.byref(n_out), int(max_kmer_occ), C.byref(cs))
        if stats is not None:
            stats.update((f, int(getattr(cs, f))) for f, _ in cs._fields_)
        if rc != 0:
            raise RuntimeError('pw_overlap_all_pairs_capped failed: ' + (lib.pw_overlap_last_error() or b'').decode())
        n = n_out.value
        pairs = np.stack([pa[:n], pb[:n]], axis=1)
        return (pairs, ps[:n], out[:n], lib.pw_overlap_last_ms()) if with_strand else (pairs, out[:n], lib.pw_overlap_last_ms())
    if with_strand:
        ps = np.zeros(max(cap, 1), np.uint8)
        rc = lib.pw_overlap_all_pairs_stranded(device, arena_c.ctypes.data, arena_c.size, roff.ctypes.data, rlen.ctypes.data, R,
                                               alphabet_len, wordlen, *coeffs, None if comp is None else comp.ctypes.data,
                                               _STRAND_SEL[strands], int(rank), int(world), cap, pa.ctypes.data, pb.ctypes.data,
                                               ps.ctypes.data, out.ctypes.data, C.byref(n_out))
        if rc != 0:
            raise RuntimeError('pw_overlap_all_pairs_stranded failed: ' + (lib.pw_overlap_last_error() or b'').decode())
        n = n_out.value
        return np.stack([pa[:n], pb[:n]], axis=1), ps[:n], out[:n], lib.pw_overlap_last_ms()
    rc = lib.pw_overlap_all_pairs(device, arena_c.ctypes.data, arena_c.size, roff.ctypes.data, rlen.ctypes.data, R, alphabet_len,
                                  wordlen, *coeffs, int(rank), int(world), cap, pa.ctypes.data, pb.ctypes.data, out.ctypes.data,
                                  C.byref(n_out))
    if rc != 0:
        raise RuntimeError('pw_overlap_all_pairs failed: ' + (lib.pw_overlap_last_error() or b'').decode())
    n = n_out.value
    return np.stack([pa[:n], pb[:n]], axis=1), out[:n], lib.pw_overlap_last_ms()


def overlap_all_pairs(reads, wordlen, alphabet, g_max, sensitivity, device=0, max_pairs=None, stats=None, strands='+',
                      complement=None, max_kmer_occ=None, minimizer_window=None):
    """The reference's all-pairs loop (``experiments/blot_overlaps.py:262-272``) in one device pass: returns a dict
    ``{(a, b): highest_scoring_overlap_band()}`` for the pairs ``a < b`` that share a seed; for every other pair the
    reference's answer is None.  With ``strands='-'`` or ``'both'`` the keys are ``(a, b, '+' | '-')`` and a minus entry
    is the reference's answer for ``reads[a]`` against the reverse complement of ``reads[b]`` (``complement``: a table or
    the ``mappings`` of ``Alphabet.transform``).

    ``max_kmer_occ`` (None or 0: no cap): k-mers that occur more often in the whole read set give no seeds
    (:func:`raw_all_pairs`), and ``stats`` also receives the cap's five counters.  With a cap no pair goes to the
    single-pair fallback -- that path knows no cap, and the reference defines no row order for a filtered seeds table:
    where ``tie > 1`` the record's own rule decides (largest ``w``, then smallest ``d``) and ``fallback_pairs`` is 0.

    ``minimizer_window`` (None, 0 or 1: no sampling): only the window minimizers of every read are indexed
    (:func:`raw_all_pairs`), and ``stats`` also receives ``positions``, ``sampled`` and ``density``.  ``p`` of every band is
    then the estimate from the sampled seeds and lies below the unsampled one: rescale a ``p_min`` of
    :func:`overlap_alignments` accordingly (``density`` is there for that); ``d_band`` is unaffected in kind.  As under the
    cap, no pair goes to the single-pair fallback: that path knows no sampling."""
    assert isinstance(alphabet, Alphabet)
    cap_stats = {}
    sampled = check_window(minimizer_window, 'minimizer_window') > 1
    cap_kw = dict(max_kmer_occ=max_kmer_occ, stats=cap_stats, minimizer_window=minimizer_window)
    if strands == '+':
        pairs, recs, ms = raw_all_pairs(reads, wordlen, len(alphabet), g_max, sensitivity, device, max_pairs, **cap_kw)
        plist = [(int(a), int(b)) for a, b in pairs.tolist()]
        res, n_fallback = _records_to_results(reads, plist, recs, wordlen, alphabet, g_max, sensitivity, device,
                                              fallback=not max_kmer_occ and not sampled)
        keys = plist
    else:
        comp = _complement(complement, len(alphabet), alphabet)
        pairs, flags, recs, ms = raw_all_pairs(reads, wordlen, len(alphabet), g_max, sensitivity, device, max_pairs, strands=strands,
                                               complement=comp, **cap_kw)
        plist = [(int(a), int(b)) for a, b in pairs.tolist()]
        res, n_fallback = _records_to_results(reads, plist, recs, wordlen, alphabet, g_max, sensitivity, device, flags, comp,
                                              fallback=not max_kmer_occ and not sampled)
        keys = [(a, b, '-' if f else '+') for (a, b), f in zip(plist, flags.tolist())]
    if stats is not None:
        stats.update(device_ms=ms, fallback_pairs=n_fallback, pairs=len(plist))
        stats.update(cap_stats)
    return dict(zip(keys, res))


def aligned_batches(arena, offs, lens, pidx, dr, alphabet_len, device=0, max_cells=2 * 10 ** 10, flags=0, strands=None,
                    complement=None, **kw):
    """Banded overlap alignment of the read pairs ``pidx`` (read indices into the packed ``arena``, :func:`pack_reads`)
    with bands ``dr``, in batches of at most ``max_cells`` cells.  The reads go to the device ONCE (``DeviceArena``) and
    every batch refers to that copy; while one batch runs on the device the next one is planned on the host
    (``pw_batch_create`` is host work: band clamps, kernel geometry, descriptors).  Yields ``(start, stop, batch)`` with
    the batch solved, traced back and synchronised; the batch is destroyed when the generator moves on.

    ``strands`` (one ``'+'`` / ``'-'`` per pair) and ``complement``: the mutant of a minus pair is the reverse complement of
    its read.  The host letters still go up once; the device writes the reverse complement of every read some minus pair
    needs behind them (``DeviceArena.with_reverse_complements``) and the batches refer to those frames as ordinary mutants."""
    from .batch import DeviceArena
    pidx = np.ascontiguousarray(pidx, np.int64).reshape(-1, 2)
    sflags = _strand_flags(strands, len(pidx))
    offs, lens = np.asarray(offs, np.int64), np.asarray(lens)
    rc_reads = np.unique(pidx[sflags == 1, 1]) if sflags is not None and sflags.any() else None
    if rc_reads is not None:
        comp = _complement(complement, alphabet_len)
        pidx = pidx.copy()
        minus = sflags == 1
        pidx[minus, 1] = len(offs) + np.searchsorted(rc_reads, pidx[minus, 1])       # the rc frames follow the reads
        lens = np.concatenate([lens, lens[rc_reads]])
    dr = np.ascontiguousarray(dr, np.int64).reshape(-1, 2)
    cells = (dr[:, 1] - dr[:, 0] + 1) * np.minimum(lens[pidx[:, 0]], lens[pidx[:, 1]]).astype(np.int64)
    bounds, start = [], 0
    csum = np.cumsum(cells)
    while start < len(pidx):
        base = csum[start - 1] if start else 0
        stop = max(start + 1, int(np.searchsorted(csum, base + max_cells, 'right')))
        bounds.append((start, stop)); start = stop

    def create(lo, hi):
        return BatchAligner.from_arena(arena, all_offs, lens, pidx[lo:hi], dr[lo:hi], device_arena=dev, alnmode=W.BANDED_MODE,
                                       alntype=W.B_OVERLAP, alphabet_len=alphabet_len, device=device, flags=flags,
                                       arena_bytes=dev.nbytes, **kw)

    if rc_reads is None:
        dev, all_offs = DeviceArena(arena, device), offs
    else:
        dev = DeviceArena.with_reverse_complements(arena, offs, lens[:len(offs)], rc_reads, comp, device)
        all_offs = np.concatenate([offs, dev.rc_offsets])
    with dev:
        cur = nxt = None
        try:
            nxt = create(*bounds[0]) if bounds else None
            for q, (lo, hi) in enumerate(bounds):
                cur, nxt = nxt, None
                cur.solve(); cur.traceback()                       # asynchronous: the device is busy from here ...
                if q + 1 < len(bounds):
                    nxt = create(*bounds[q + 1])                   # ... while the next batch is planned
                cur.sync()
                yield lo, hi, cur
                cur.close(); cur = None
        finally:
            for b in (cur, nxt):
                if b is not None:
                    b.close()


def overlap_alignments(reads, pairs, bands, alphabet, p_min=0., device=0, max_cells=2 * 10 ** 10, want_transcripts=True,
                       strands=None, complement=None, want_summaries=False, pileup=None, pileup_sides='origin', graph=None, **aligner_kw):
    """Banded overlap alignment (``B_OVERLAP``) of every pair whose band has ``p >= p_min``; the ``diag_range`` is the
    band clamped to the table as ``Aligner`` requires (``pw.py:224-226``).  All reads are uploaded ONCE and the pairs
    refer to them (``BatchAligner.from_arena``); the pairs are solved in batches of at most ``max_cells`` cells
    (tie masks take 0.5-0.6 bytes per cell of HBM).  ``bands`` is a list aligned with ``pairs`` (dicts or None).
    Returns a list with one entry per pair: None, or dict(score, transcript, origin_start, mutant_start,
    diag_range).  With ``strands`` (one ``'+'`` / ``'-'`` per pair; ``complement`` as in :func:`overlap_bands`) the mutant
    of a minus pair is the reverse complement of ``reads[j]``, ``mutant_start`` and the transcript are in its frame
    (:func:`minus_to_forward`), and every dict also reports its ``strand``.  With ``want_summaries`` every dict gains
    ``summary``: the op counts, gap runs and match bounds of its transcript (the fields of ``batch.SUMMARY_DTYPE``, in the
    transcript's own frame), reduced on the device -- with or without ``want_transcripts``.

    ``pileup``: None, or a :class:`biseqt_amd.batch.Pileup` that spans the arena of ``pack_reads(reads)`` -- ``n_cols`` is the
    size of that arena in bytes, ``alphabet_len`` the alphabet's.  Every batch then adds its pairs onto their ORIGIN reads
    (:meth:`BatchAligner.pileup_add` with ``arena_first = 0`` and no ``col0``), with or without ``want_transcripts``: read
    ``a`` of a pair ``(a, b)`` is always in its forward frame, minus strand included, where the letters piled onto it are
    those of ``rc(reads[b])``.  With ``arena, offs, lens = pack_reads(reads)``, letter ``x`` of read ``r`` is column
    ``offs[r] + x``: the columns of read ``r`` are ``pileup.counts(offs[r], offs[r] + lens[r])``; the columns between two
    reads (alignment padding) stay zero.  The caller owns the pileup.

    ``pileup_sides``: ``'origin'`` (the above) or ``'both'`` (include/pw_polish.h): every batch also adds pair ``(a, b)`` onto
    read ``b``, at ``mutant_col0 = offs[b]``, and reversed for a minus pair -- the batch itself only knows the frame of
    ``rc(reads[b])`` behind the arena -- so that the columns of read ``b`` are always its forward letters.  The inserted
    letters go to the insertion plane of a pileup that has one (``Pileup(..., ins_slots=J)``).

    ``graph``: None, or an open :class:`biseqt_amd.graph.OverlapGraph` over the lengths of ``reads``: every batch appends one
    overlap record per pair it aligned (include/pw_graph.h) -- read ``a``, read ``b`` and the strand flag of the pair -- with or
    without ``want_transcripts``; a pair without an alignment gives a ``NONE`` record.  The caller owns the graph."""
    from .batch import Pileup, pack_reads, summary_dict
    if pileup_sides not in ('origin', 'both'):
        raise ValueError("pileup_sides is 'origin' or 'both', not %r" % (pileup_sides,))
    arena, offs, lens = pack_reads(reads)
    if pileup is not None:
        if not isinstance(pileup, Pileup) or not pileup.handle:
            raise ValueError('pileup must be an open biseqt_amd.batch.Pileup')
        if pileup.n_cols != arena.nbytes or pileup.alphabet_len != len(alphabet) or pileup.device != device:
            raise ValueError('pileup must span the arena of pack_reads(reads): n_cols == %d, alphabet_len %d, on device %d'
                             % (arena.nbytes, len(alphabet), device))
    if graph is not None:
        from .graph import OverlapGraph
        if not isinstance(graph, OverlapGraph) or not graph.handle:
            raise ValueError('graph must be an open biseqt_amd.graph.OverlapGraph')
        if graph.device != device or graph.n_reads != len(lens) or (graph.read_lens != lens).any():
            raise ValueError('graph must hold the lengths of `reads`, on device %d' % device)
    sflags = _strand_flags(strands, len(pairs))
    comp = _complement(complement, len(alphabet), alphabet) if sflags is not None and sflags.any() else None
    sel, dr = [], []
    for q, ((i, j), band) in enumerate(zip(pairs, bands)):
        if band is None or band['p'] < p_min:
            continue
        lo = max(int(band['d_band'][0]), -int(lens[j]))
        hi = min(int(band['d_band'][1]), int(lens[i]))
        if lo > hi:
            continue
        sel.append(q); dr.append((lo, hi))
    out = [None] * len(pairs)
    if not sel:
        return out
    kw = dict(match_score=1, mismatch_score=-3, go_score=-5, ge_score=-2)
    kw.update(aligner_kw)
    pidx = np.array([pairs[q] for q in sel], np.int64)
    dr = np.array(dr, np.int64)
    sub = None if sflags is None else sflags[sel]
    for start, stop, b in aligned_batches(arena, offs, lens, pidx, dr, len(alphabet), device=device, max_cells=max_cells,
                                          strands=sub, complement=comp, **kw):
        res = b.results()
        txs = b.transcripts(res) if want_transcripts else [None] * (stop - start)
        sums = b.summaries() if want_summaries else None
        if pileup is not None:
            if pileup_sides == 'both':
                b.pileup_add(pileup, sides='both', mutant_col0=offs[pidx[start:stop, 1]],
                             reverse=None if sub is None else sub[start:stop], complement=comp)
            else:
                b.pileup_add(pileup)
            b.sync()                                               # (the batch goes when the generator moves on)
        if graph is not None:
            graph.add_batch(b, pidx[start:stop, 0], pidx[start:stop, 1], None if sub is None else sub[start:stop])
            b.sync()
        for k in range(stop - start):
            if res['opt_i'][k] < 0:
                continue
            out[sel[start + k]] = dict(score=float(res['score'][k]), transcript=txs[k], origin_start=int(res['origin_idx'][k]),
                                       mutant_start=int(res['mutant_idx'][k]), diag_range=(int(dr[start + k, 0]), int(dr[start + k, 1])))
            if sub is not None:
                out[sel[start + k]]['strand'] = '-' if sub[start + k] else '+'
            if sums is not None:
                out[sel[start + k]]['summary'] = summary_dict(sums[k])
    return out


def polish_reads(reads, pairs, bands, alphabet, p_min=0., strands=None, complement=None, min_depth=3, ins_slots=2, self_weight=1,
                 device=0, stats=None, **aligner_kw):
    """Read correction from overlaps that are known (include/pw_polish.h): the reads are packed, every read votes for its own
    letters with ``self_weight``, :func:`overlap_alignments` piles every aligned pair onto BOTH of its reads
    (``pileup_sides='both'``, no transcript leaves the device) into a pileup with ``ins_slots`` insertion slots, and the
    pileup is polished with ``min_depth``.  ``pairs``, ``bands``, ``p_min``, ``strands``, ``complement`` and ``aligner_kw``
    are :func:`overlap_alignments`'.  Returns the corrected reads as uint8 arrays, in read order.  ``stats`` (a dict)
    receives ``records`` (one ``batch.POLISH_STATS_DTYPE`` record per read), ``aligned`` (pairs with an alignment) and the
    times of the three device stages in ms, taken on the host around synchronised device work: ``vote_ms``, ``align_ms``
    (alignment and two-sided adds), ``polish_ms``."""
    import time
    from .batch import DeviceArena, Pileup, pack_reads
    assert isinstance(alphabet, Alphabet)
    arena, offs, lens = pack_reads(reads)
    letters = np.full(arena.nbytes, 255, np.uint8)             # the padding between two reads votes for nothing
    for o, n in zip(offs.tolist(), lens.tolist()):
        letters[o:o + n] = arena[o:o + n]
    with Pileup(arena.nbytes, len(alphabet), device=device, ins_slots=ins_slots) as pile, DeviceArena(letters, device) as dev:
        t0 = time.perf_counter()
        pile.add_letters((dev, 0), weight=self_weight)
        dev.read(0, 1)                                         # (a synchronous copy behind the vote)
        t1 = time.perf_counter()
        alns = overlap_alignments(reads, pairs, bands, alphabet, p_min=p_min, device=device, want_transcripts=False, strands=strands,
                                  complement=complement, pileup=pile, pileup_sides='both', **aligner_kw)
        t2 = time.perf_counter()
        out, offsets, records = pile.polish((dev, 0), offs, lens, min_depth=min_depth)
        t3 = time.perf_counter()
    if stats is not None:
        stats.update(records=records, aligned=sum(a is not None for a in alns), vote_ms=1e3 * (t1 - t0), align_ms=1e3 * (t2 - t1),
                     polish_ms=1e3 * (t3 - t2))
    return [out[offsets[r]:offsets[r + 1]].copy() for r in range(len(lens))]


def correct_reads(reads, wordlen, alphabet, g_max, sensitivity, p_min=.8, strands='+', complement=None, minimizer_window=None,
                  max_kmer_occ=None, max_pairs=None, min_depth=3, ins_slots=2, self_weight=1, device=0, stats=None, **aligner_kw):
    """From reads to corrected reads in one call: :func:`overlap_all_pairs` (``strands``, ``complement``, ``minimizer_window``,
    ``max_kmer_occ``, ``max_pairs`` are its arguments), then :func:`polish_reads` on the pairs it found whose band has
    ``p >= p_min`` (under minimizer sampling ``p`` is the estimate from the sampled seeds: rescale ``p_min``).  ``stats``
    receives what both stages report, the overlap stage's under ``overlaps``."""
    ostats = {}
    found = overlap_all_pairs(reads, wordlen, alphabet, g_max, sensitivity, device=device, max_pairs=max_pairs, stats=ostats,
                              strands=strands, complement=complement, max_kmer_occ=max_kmer_occ, minimizer_window=minimizer_window)
    keys = list(found)
    pairs = [(k[0], k[1]) for k in keys]
    pstrands = [k[2] for k in keys] if strands != '+' else None
    if stats is not None:
        stats['overlaps'] = ostats
    return polish_reads(reads, pairs, [found[k] for k in keys], alphabet, p_min=p_min, strands=pstrands, complement=complement,
                        min_depth=min_depth, ins_slots=ins_slots, self_weight=self_weight, device=device, stats=stats, **aligner_kw)


def assemble_reads(reads, wordlen, alphabet, g_max, sensitivity, p_min=.8, strands='+', complement=None, minimizer_window=None,
                   max_kmer_occ=None, stats=None, max_hang=1000, int_frac=.8, min_overlap=0, min_identity=0., fuzz=10, device=0,
                   consensus=False, slack=50, drift=.1, min_depth=3, ins_slots=2, self_weight=1, max_tip_reads=0, max_bubble_reads=0,
                   clean_rounds=1, consensus_rounds=1, **aligner_kw):
    """From reads to contigs in one call (include/pw_graph.h): :func:`overlap_all_pairs` (``strands``, ``complement``,
    ``minimizer_window``, ``max_kmer_occ`` are its arguments), :func:`overlap_alignments` of the pairs it found whose band has
    ``p >= p_min`` into an :class:`biseqt_amd.graph.OverlapGraph` (no transcript leaves the device), its ``build`` with
    ``max_hang``, ``int_frac``, ``min_overlap``, ``min_identity``, ``fuzz``, and its ``contigs``.  Returns ``(contigs, unitigs,
    members, contained)``: the contig letters as uint8 arrays, the ``graph.UNITIG_DTYPE`` and ``graph.MEMBER_DTYPE`` records and
    one byte per read.  Without ``consensus`` the contig letters are those of single reads, one after another: correct the
    reads first (:func:`correct_reads`), or ask for the consensus.  ``stats`` (a dict) receives the
    overlap stage's report under ``overlaps``, ``records`` (the overlap records with their classes), ``aligned``, ``arcs``,
    ``kept_arcs``, ``device_bytes`` and the times of the stages in ms, taken on the host around synchronised device work:
    ``overlap_ms``, ``align_ms``, ``build_ms``, ``contigs_ms``.

    ``max_tip_reads``, ``max_bubble_reads``, ``clean_rounds`` go to ``build`` (the CLEANING of include/pw_graph.h: tips and the
    weaker of parallel paths are dropped before the unitigs are laid out; off by default).  ``stats`` gains ``dropped``: a dict
    of ``reads`` (one byte per read: 1 tip, 2 bubble), ``tips`` and ``bubbles`` (their counts).

    ``consensus=True`` (include/pw_consensus.h): the first element holds the POLISHED contigs instead --
    :meth:`biseqt_amd.graph.OverlapGraph.consensus` with ``slack``, ``drift``, ``min_depth``, ``ins_slots``, ``self_weight`` and the
    same ``aligner_kw``: every read, the contained ones included, is placed on its contig, realigned against the draft and
    piled onto it.  ``stats`` then gains ``draft`` (the unpolished letters, what the call returns without ``consensus``),
    ``placements`` (``graph.PLACE_DTYPE``), ``consensus_records`` (one ``batch.POLISH_STATS_DTYPE`` record per contig),
    ``consensus_stats`` (``placed``, ``unplaced``, ``tasks``, ``aligned``) and ``layout_ms``, ``consensus_align_ms``, ``polish_ms``.
    ``consensus_rounds`` is the consensus's ``rounds`` (include/pw_rounds.h: the polished contigs are laid out, realigned and
    polished again, until a round changes nothing); ``stats['consensus_rounds']`` holds its per-round list."""
    import time
    from .graph import ARC_REMOVED, OverlapGraph
    assert isinstance(alphabet, Alphabet)
    ostats = {}
    t0 = time.perf_counter()
    found = overlap_all_pairs(reads, wordlen, alphabet, g_max, sensitivity, device=device, stats=ostats, strands=strands,
                              complement=complement, max_kmer_occ=max_kmer_occ, minimizer_window=minimizer_window)
    keys = list(found)
    pairs = [(k[0], k[1]) for k in keys]
    pstrands = [k[2] for k in keys] if strands != '+' else None
    comp = _complement(complement, len(alphabet), alphabet) if strands != '+' else None
    t1 = time.perf_counter()
    with OverlapGraph([len(r) for r in reads], device=device) as G:
        alns = overlap_alignments(reads, pairs, [found[k] for k in keys], alphabet, p_min=p_min, device=device, want_transcripts=False,
                                  strands=pstrands, complement=complement, graph=G, **aligner_kw)
        t2 = time.perf_counter()
        G.build(max_hang=max_hang, int_frac=int_frac, min_overlap=min_overlap, min_identity=min_identity, fuzz=fuzz,
                max_tip_reads=max_tip_reads, max_bubble_reads=max_bubble_reads, clean_rounds=clean_rounds)
        t3 = time.perf_counter()
        contigs = G.contigs(reads, complement=comp)
        t4 = time.perf_counter()
        unitigs, members = G.unitigs()
        contained = G.contained()
        if consensus:
            cstats = {}
            draft = contigs
            contigs, crecords = G.consensus(reads, len(alphabet), complement=comp, slack=slack, drift=drift, min_depth=min_depth,
                                            ins_slots=ins_slots, self_weight=self_weight, stats=cstats, rounds=consensus_rounds, **aligner_kw)
            if stats is not None:
                stats.update(draft=draft, placements=G.placements(), consensus_records=crecords,
                             consensus_stats={k: cstats[k] for k in ('placed', 'unplaced', 'tasks', 'aligned')},
                             layout_ms=cstats['layout_ms'], consensus_align_ms=cstats['align_ms'], polish_ms=cstats['polish_ms'],
                             consensus_rounds=cstats['rounds'])
        if stats is not None:
            arcs, _ = G.arcs()
            gone = G.dropped()
            stats['dropped'] = dict(reads=gone, tips=int((gone == 1).sum()), bubbles=int((gone == 2).sum()))
            stats.update(overlaps=ostats, records=G.overlaps(), aligned=sum(a is not None for a in alns), arcs=len(arcs),
                         kept_arcs=int((arcs['flags'] & ARC_REMOVED == 0).sum()), device_bytes=G.device_bytes,
                         overlap_ms=1e3 * (t1 - t0), align_ms=1e3 * (t2 - t1), build_ms=1e3 * (t3 - t2), contigs_ms=1e3 * (t4 - t3))
    return contigs, unitigs, members, contained


def raw_bands_sharded(reads, pairs, wordlen, alphabet_len, g_max, sensitivity, rank, world, device=None, gather_device=None,
                      strands=None, complement=None):
    """Config 4 across GPUs: pair q is scored by rank ``q mod world`` (no data-path collective), the 64-byte band
    records are gathered to rank 0 in pair order (``torch.distributed``: RCCL on GPUs).  Returns the full record
    array on rank 0, None elsewhere."""
    from .distributed import gather_struct, shard_indices
    mine = shard_indices(len(pairs), rank, world)
    flags = _strand_flags(strands, len(pairs))
    recs, _ = raw_bands(reads, [pairs[q] for q in mine], wordlen, alphabet_len, g_max, sensitivity,
                        device=rank if device is None else device, strands=None if flags is None else flags[list(mine)],
                        complement=complement)
    return gather_struct(recs, len(pairs), rank, world, device=gather_device)


def raw_all_pairs_sharded(reads, wordlen, alphabet_len, g_max, sensitivity, rank, world, device=None, max_pairs=None, strands='+',
                          complement=None, max_kmer_occ=None, stats=None, minimizer_window=None):
    """Config 4 across GPUs: every rank indexes all reads (cheap) and joins / scores the pairs whose smaller read
    index is ``rank`` modulo ``world``; pair lists and 64-byte records are gathered to rank 0 (ragged byte gather over
    ``torch.distributed``) and merged in ascending (a, b) order.  Returns ``(pairs, records)`` on rank 0, None elsewhere.
    With ``strands`` other than ``'+'``: ``(pairs, strand, records)`` in ascending (a, b, strand) order.
    ``max_kmer_occ`` / ``stats``: the occurrence cap of :func:`raw_all_pairs`, counted over the whole read set on every rank, so
    the merged output equals the unsharded capped call's; ``stats`` receives THIS rank's counters.
    ``minimizer_window``: the sampling of :func:`raw_all_pairs`; every rank samples the whole read set, so the merged output
    equals the unsharded sampled call's."""
    import torch
    from .distributed import gather_bytes
    if strands != '+':
        return _raw_all_pairs_sharded_stranded(reads, wordlen, alphabet_len, g_max, sensitivity, rank, world, device, max_pairs,
                                               strands, complement, max_kmer_occ, stats, minimizer_window)
    pairs, recs, _ = raw_all_pairs(reads, wordlen, alphabet_len, g_max, sensitivity, device=rank if device is None else device,
                                   max_pairs=max_pairs, rank=rank, world=world, max_kmer_occ=max_kmer_occ, stats=stats,
                                   minimizer_window=minimizer_window)
    blob = np.concatenate([np.ascontiguousarray(pairs, np.int32).view(np.uint8).reshape(-1), recs.view(np.uint8).reshape(-1)])
    got = gather_bytes(torch.from_numpy(blob.copy()), rank, world)
    if rank != 0:
        return None
    all_pairs, all_recs = [], []
    for t in got:
        raw = t.cpu().numpy()
        n = raw.size // (8 + BAND_DTYPE.itemsize)
        all_pairs.append(raw[:8 * n].view(np.int32).reshape(n, 2))
        all_recs.append(raw[8 * n:].view(BAND_DTYPE))
    pairs, recs = np.concatenate(all_pairs), np.concatenate(all_recs)
    order = np.lexsort((pairs[:, 1], pairs[:, 0]))
    return pairs[order], recs[order]


def _raw_all_pairs_sharded_stranded(reads, wordlen, alphabet_len, g_max, sensitivity, rank, world, device, max_pairs, strands,
                                    complement, max_kmer_occ=None, stats=None, minimizer_window=None):
    """:func:`raw_all_pairs_sharded` with the strand column: the third int32 of every gathered pair."""
    import torch
    from .distributed import gather_bytes
    pairs, flags, recs, _ = raw_all_pairs(reads, wordlen, alphabet_len, g_max, sensitivity, device=rank if device is None else device,
                                          max_pairs=max_pairs, rank=rank, world=world, strands=strands, complement=complement,
                                          max_kmer_occ=max_kmer_occ, stats=stats, minimizer_window=minimizer_window)
    triples = np.ascontiguousarray(np.concatenate([pairs, flags.astype(np.int32)[:, None]], axis=1), np.int32)
    blob = np.concatenate([triples.view(np.uint8).reshape(-1), recs.view(np.uint8).reshape(-1)])
    got = gather_bytes(torch.from_numpy(blob.copy()), rank, world)
    if rank != 0:
        return None
    all_triples, all_recs = [], []
    for t in got:
        raw = t.cpu().numpy()
        n = raw.size // (12 + BAND_DTYPE.itemsize)
        all_triples.append(raw[:12 * n].view(np.int32).reshape(n, 3))
        all_recs.append(raw[12 * n:].view(BAND_DTYPE))
    triples, recs = np.concatenate(all_triples), np.concatenate(all_recs)
    order = np.lexsort((triples[:, 2], triples[:, 1], triples[:, 0]))
    return triples[order, :2], triples[order, 2].astype(np.uint8), recs[order]
