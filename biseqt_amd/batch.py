"""Batches of independent alignment problems on one GPU (host side of include/pw_batch.h).

No reference counterpart: the reference solves one pair per ``Aligner`` (``biseqt/pw.py:119-319``).
Per pair a batch computes exactly what ``Aligner.solve()`` + ``Aligner.traceback()`` compute, for
all pairs in a handful of kernel launches.  Keyword arguments keep the reference's names
(``alnmode``, ``alntype``, ``subst_scores``, ``match_score``, ``mismatch_score``, ``go_score``,
``ge_score``, ``diag_range``).
"""
import ctypes as C

import numpy as np

from . import _pwlib as W
from .sequence import Sequence

RESULT_DTYPE = np.dtype([('score', '<f8'), ('opt_i', '<i4'), ('opt_j', '<i4'),
                         ('origin_idx', '<i4'), ('mutant_idx', '<i4'),
                         ('tx_len', '<i4'), ('status', '<i4')])
assert RESULT_DTYPE.itemsize == 32
# pw_tx_summary of include/pw_txsum.h: what a transcript holds, reduced on the device
SUMMARY_DTYPE = np.dtype([(f, '<i4') for f in ('n_match', 'n_subst', 'n_ins', 'n_del', 'n_gaps', 'first_match', 'last_match',
                                               'head_origin', 'head_mutant', 'tail_origin', 'tail_mutant', 'flags')])
assert SUMMARY_DTYPE.itemsize == 48
# include/pw_cigar.h: a run is one uint32, (length << 4) | op with BAM's op codes
CIGAR_EXTENDED, CIGAR_CLASSIC = W.PW_CIGAR_EXTENDED, W.PW_CIGAR_CLASSIC
CIGAR_OPS = 'MIDNSHP=X'
_CIGAR_FORMS = {'extended': CIGAR_EXTENDED, 'classic': CIGAR_CLASSIC}
# pw_pileup_site of include/pw_pileup.h: one called column of a pileup
SITE_DTYPE = np.dtype([('depth', '<u4'), ('call', 'u1'), ('ref', 'u1'), ('flags', '<u2')])
assert SITE_DTYPE.itemsize == 8
# pw_polish_stats of include/pw_polish.h: what became of the columns of one polished read
POLISH_STATS_DTYPE = np.dtype([(f, '<u4') for f in ('kept', 'substituted', 'deleted', 'inserted')])
assert POLISH_STATS_DTYPE.itemsize == 16
_SIDES = {'origin': W.PW_SIDE_ORIGIN, 'mutant': W.PW_SIDE_MUTANT, 'both': W.PW_SIDE_BOTH}
_CIGAR_LETTERS = ({'M': '=', 'S': 'X', 'I': 'I', 'D': 'D'}, {'M': 'M', 'S': 'M', 'I': 'I', 'D': 'D'})


def _cigar_form(form):
    """``'extended'`` / ``'classic'`` (or the constants) -> PW_CIGAR_EXTENDED / PW_CIGAR_CLASSIC."""
    if isinstance(form, str) and form in _CIGAR_FORMS:
        return _CIGAR_FORMS[form]
    if not isinstance(form, (str, bool)) and form in (CIGAR_EXTENDED, CIGAR_CLASSIC):
        return int(form)
    raise ValueError("form is 'extended' or 'classic', not %r" % (form,))


def _as_u8(seq):
    if isinstance(seq, Sequence):
        return seq.as_array(np.uint8)
    a = np.asarray(seq)
    assert a.ndim == 1
    if a.size:
        assert a.min() >= 0 and a.max() <= 255, 'letters must be 0..255'
    return np.ascontiguousarray(a, dtype=np.uint8)


class DeviceBuffer(object):
    """A view of device memory owned by a batch, exportable to torch without a copy
    (``torch.as_tensor(buf, device='cuda')``) through ``__cuda_array_interface__``."""

    def __init__(self, ptr, nbytes, owner):
        self.ptr, self.nbytes, self.owner = ptr, nbytes, owner

    @property
    def __cuda_array_interface__(self):
        return dict(shape=(self.nbytes,), typestr='|u1', data=(self.ptr, False), version=2)


class PinnedArray(object):
    """Page-locked host memory (``pw_host_alloc``) viewed as a numpy array: the source / destination of the
    asynchronous transfers (``upload_async``, ``results_async``, ``transcripts_async``)."""

    def __init__(self, nbytes, dtype=np.uint8):
        self.lib = W.load()
        self.nbytes = int(nbytes)
        self.ptr = self.lib.pw_host_alloc(max(self.nbytes, 1))
        if not self.ptr:
            raise MemoryError('pw_host_alloc(%d) failed: %s' % (nbytes, W.last_error()))
        buf = (C.c_uint8 * max(self.nbytes, 1)).from_address(self.ptr)
        self.array = np.frombuffer(buf, dtype=np.uint8, count=self.nbytes).view(dtype)

    def close(self):
        if getattr(self, 'ptr', None):
            self.array = None
            self.lib.pw_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


PAIR_DTYPE = np.dtype([('origin_off', '<u8'), ('mutant_off', '<u8'), ('origin_len', '<i4'), ('mutant_len', '<i4'),
                       ('dmin', '<i4'), ('dmax', '<i4')])
assert PAIR_DTYPE.itemsize == 32


def pack_reads(reads):
    """All reads once in one letter arena, every read on a 16-byte boundary (frames must be 4-byte aligned, with
    slack behind): returns ``(arena uint8, offsets int64, lengths int32)`` for :meth:`BatchAligner.from_arena`."""
    arrs = [_as_u8(r) for r in reads]
    lens = np.array([len(a) for a in arrs], np.int64)
    sizes = (lens + 15) // 16 * 16 + 16
    offs = np.zeros(len(arrs), np.int64)
    if len(arrs):
        offs[1:] = np.cumsum(sizes)[:-1]
    arena = np.zeros(int(sizes.sum()) + 16, np.uint8)
    for a, o in zip(arrs, offs):
        arena[o:o + len(a)] = a
    return arena, offs, lens.astype(np.int32)


class DeviceArena(object):
    """One device copy of a read arena (:func:`pack_reads`) for all the batches of a job (``pw_arena_upload``)."""

    def __init__(self, arena, device=0):
        self.lib = W.load()
        arena = np.ascontiguousarray(arena, np.uint8)
        self.device, self.nbytes = device, arena.nbytes
        self.ptr = self.lib.pw_arena_upload(device, arena.ctypes.data, arena.nbytes)
        if not self.ptr:
            raise RuntimeError('pw_arena_upload failed: ' + W.last_error())

    @classmethod
    def with_reverse_complements(cls, arena, offsets, lengths, which, complement, device=0):
        """The arena uploaded once, and behind it the reverse complements of the reads ``which`` (indices into ``offsets`` /
        ``lengths``), written by the device from the forward letters (``pw_overlap_arena_upload``) with the frame alignment
        and slack of :func:`pack_reads`.  ``rc_offsets[q]`` is the offset of ``rc(reads[which[q]])``; ``nbytes`` covers the
        forward and the reverse-complement frames, so a batch refers to either kind as an ordinary frame."""
        self = cls.__new__(cls)
        self.lib = W.load()
        arena = np.ascontiguousarray(arena, np.uint8)
        which = np.ascontiguousarray(which, np.int64).reshape(-1)
        comp = np.ascontiguousarray(complement, np.uint8)
        offsets, lengths = np.asarray(offsets, np.int64), np.asarray(lengths, np.int64)
        src = np.ascontiguousarray(offsets[which].astype(np.uint64))
        ln = np.ascontiguousarray(lengths[which].astype(np.int32))
        sizes = (lengths[which] + 15) // 16 * 16 + 16
        base = (arena.nbytes + 15) // 16 * 16
        dst = np.zeros(len(which), np.uint64)
        if len(which):
            dst[:] = base + np.concatenate([[0], np.cumsum(sizes)[:-1]])
        total = int(base + sizes.sum() + 16)
        self.device, self.nbytes, self.rc_offsets = device, total, dst.astype(np.int64)
        self.ptr = self.lib.pw_overlap_arena_upload(device, arena.ctypes.data, arena.nbytes, total, len(which), src.ctypes.data,
                                                    dst.ctypes.data, ln.ctypes.data, comp.ctypes.data, len(comp))
        if not self.ptr:
            raise RuntimeError('pw_overlap_arena_upload failed: ' + (self.lib.pw_overlap_last_error() or b'').decode())
        return self

    @classmethod
    def adopt(cls, ptr, nbytes, device=0, owner=None):
        """A non-owning view of ``nbytes`` bytes of device memory at ``ptr`` that somebody else owns (``owner``, kept alive as
        long as the view): frames of it serve batches, pileups and :meth:`read` as those of an uploaded arena do, and
        :meth:`close` never frees the pointer.  The memory must carry the 16 bytes of slack behind ``nbytes`` that
        ``pw_arena_upload`` gives."""
        if not ptr or int(nbytes) < 0:
            raise ValueError('adopt needs a device pointer and a size')
        self = cls.__new__(cls)
        self.lib = W.load()
        self.device, self.nbytes, self.ptr = device, int(nbytes), int(ptr)
        self._adopted, self._owner = True, owner
        return self

    def read(self, offset=0, nbytes=None):
        """A piece of the device arena back on the host (uint8 array)."""
        nbytes = self.nbytes - offset if nbytes is None else nbytes
        assert 0 <= offset and offset + nbytes <= self.nbytes
        out = np.zeros(max(nbytes, 1), np.uint8)
        if self.lib.pw_overlap_arena_read(self.device, self.ptr, offset, nbytes, out.ctypes.data) != 0:
            raise RuntimeError('pw_overlap_arena_read failed: ' + (self.lib.pw_overlap_last_error() or b'').decode())
        return out[:nbytes]

    def close(self):
        if getattr(self, '_adopted', False):                # (an adopted pointer belongs to its owner)
            self.ptr = self._owner = None
            return
        if self.ptr:
            self.lib.pw_arena_free(self.device, self.ptr)
            self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Pileup(object):
    """Per-column base counts of the origins of many alignments, device-resident (include/pw_pileup.h): ``uint32
    counts[n_cols][alphabet_len + 2]`` -- one channel per letter, then ``DEL`` (the ``D`` ops over the column) and ``INS`` (the
    insertion events anchored to the column on their left) -- zeroed at creation and filled by
    :meth:`BatchAligner.pileup_add` from the transcripts where the traceback left them.  The header has the definition op by
    op.  A cell wraps past ``2**32 - 1``; keeping the depth below that is the caller's business.  A context manager that
    frees itself, like :class:`DeviceArena`.

    With ``ins_slots = J`` in 1 .. 8 the pileup also owns the insertion plane of include/pw_polish.h, ``uint32
    ins[n_cols][J][alphabet_len]``: the first ``J`` letters of every insertion run, per column and slot, filled by
    :meth:`BatchAligner.pileup_add` with ``sides=`` and read by :meth:`polish`."""

    def __init__(self, n_cols, alphabet_len, device=0, ins_slots=0):
        self.handle = None
        n_cols, alphabet_len, ins_slots = int(n_cols), int(alphabet_len), int(ins_slots)
        if not 1 <= alphabet_len <= 32:
            raise ValueError('alphabet_len must be 1..32, not %d' % alphabet_len)
        if n_cols < 0:
            raise ValueError('n_cols must not be negative')
        if not 0 <= ins_slots <= W.PW_POLISH_MAX_SLOTS:
            raise ValueError('ins_slots must be 0 (no insertion plane) or 1..8, not %d' % ins_slots)
        self.lib = W.load()
        self.n_cols, self.alphabet_len, self.device, self.ins_slots = n_cols, alphabet_len, device, ins_slots
        self.DEL, self.INS = alphabet_len, alphabet_len + 1
        self._ref = None                     # the device copy of a host reference given to call(): alive as long as the sites
        if ins_slots:
            self.handle = self.lib.pw_pileup_create_ins(device, n_cols, alphabet_len, ins_slots)
        else:
            self.handle = self.lib.pw_pileup_create(device, n_cols, alphabet_len)
        if not self.handle:
            raise RuntimeError('%s failed: %s' % ('pw_pileup_create_ins' if ins_slots else 'pw_pileup_create', W.last_error()))

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.pw_pileup_destroy(self.handle)
            self.handle = None
        if getattr(self, '_ref', None) is not None:
            self._ref.close()
            self._ref = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        if rc != 0:
            raise RuntimeError('%s failed: %s' % (what, W.last_error()))

    def _range(self, lo, hi):
        hi = self.n_cols if hi is None else int(hi)
        lo = int(lo)
        if not 0 <= lo <= hi <= self.n_cols:
            raise ValueError('columns [%d, %d) outside the pileup of %d' % (lo, hi, self.n_cols))
        return lo, hi

    def clear(self, stream=None):
        """All counts back to zero (asynchronous on ``stream``)."""
        self._ck(self.lib.pw_pileup_clear(self.handle, stream), 'pw_pileup_clear')

    def counts(self, lo=0, hi=None):
        """``uint32[hi - lo, alphabet_len + 2]`` of the columns ``[lo, hi)`` (synchronous D2H)."""
        lo, hi = self._range(lo, hi)
        out = np.zeros((hi - lo, self.alphabet_len + 2), np.uint32)
        self._ck(self.lib.pw_pileup_counts(self.handle, lo, hi, out.ctypes.data), 'pw_pileup_counts')
        return out

    def set_counts(self, counts, lo=0):
        """Overwrite the columns ``[lo, lo + len(counts))`` with host counts: a pileup saved earlier, or one summed over
        several devices (synchronous H2D)."""
        a = np.ascontiguousarray(counts, np.uint32)
        if a.ndim != 2 or a.shape[1] != self.alphabet_len + 2:
            raise ValueError('counts must be [columns, alphabet_len + 2]')
        lo, hi = self._range(lo, int(lo) + len(a))
        self._ck(self.lib.pw_pileup_set_counts(self.handle, lo, hi, a.ctypes.data), 'pw_pileup_set_counts')

    def counts_device(self):
        return DeviceBuffer(self.lib.pw_pileup_counts_device(self.handle), 4 * self.n_cols * (self.alphabet_len + 2), self)

    def call(self, ref=None, min_depth=1, stream=None):
        """One :data:`SITE_DTYPE` record per column from the counts as they are (``pw_pileup_call``, asynchronous on ``stream``):
        ``depth`` (letters + ``DEL``), ``call`` (the channel with the largest count, a tie to the lowest; 255 below
        ``min_depth`` or at depth 0), ``ref`` and ``flags`` (``PW_PILEUP_COVERED | DIFFERS | INSERT``).  ``ref``: None, a host
        array of ``n_cols`` letters (uploaded here), or ``(DeviceArena, offset)`` for letters that are on the device already."""
        min_depth = int(min_depth)
        if not 0 <= min_depth < 1 << 32:
            raise ValueError('min_depth must fit 32 bits')
        ptr, held = None, None
        if isinstance(ref, tuple):
            arena, off = ref
            if not isinstance(arena, DeviceArena) or arena.device != self.device or not 0 <= int(off) <= arena.nbytes - self.n_cols:
                raise ValueError('ref is (DeviceArena on device %d, offset) with n_cols letters behind the offset' % self.device)
            ptr = arena.ptr + int(off)
        elif ref is not None:
            letters = _as_u8(ref)
            if len(letters) != self.n_cols:
                raise ValueError('ref has %d letters, the pileup %d columns' % (len(letters), self.n_cols))
            held = DeviceArena(letters if len(letters) else np.zeros(1, np.uint8), device=self.device)
            ptr = held.ptr
        self._ck(self.lib.pw_pileup_call(self.handle, ptr, min_depth, stream), 'pw_pileup_call')
        if self._ref is not None:
            self._ref.close()                # (pw_arena_free waits for the device: an earlier call has read it by now)
        self._ref = held

    def sites(self, lo=0, hi=None):
        """Structured array (:data:`SITE_DTYPE`) of the columns ``[lo, hi)`` as the last :meth:`call` left them (synchronous D2H)."""
        lo, hi = self._range(lo, hi)
        out = np.zeros(hi - lo, SITE_DTYPE)
        self._ck(self.lib.pw_pileup_sites(self.handle, lo, hi, out.ctypes.data), 'pw_pileup_sites')
        return out

    def sites_device(self):
        ptr = self.lib.pw_pileup_sites_device(self.handle)
        if not ptr:
            raise RuntimeError('sites_device before call')
        return DeviceBuffer(ptr, 8 * self.n_cols, self)

    # ---- read correction (include/pw_polish.h) ----
    def ins_counts(self, lo=0, hi=None):
        """``uint32[hi - lo, ins_slots, alphabet_len]`` of the insertion plane's columns ``[lo, hi)`` (synchronous D2H)."""
        lo, hi = self._range(lo, hi)
        if not self.ins_slots:
            raise ValueError('the pileup has no insertion plane (ins_slots=0)')
        out = np.zeros((hi - lo, self.ins_slots, self.alphabet_len), np.uint32)
        self._ck(self.lib.pw_pileup_ins_counts(self.handle, lo, hi, out.ctypes.data), 'pw_pileup_ins_counts')
        return out

    def ins_counts_device(self):
        if not self.ins_slots:
            raise ValueError('the pileup has no insertion plane (ins_slots=0)')
        return DeviceBuffer(self.lib.pw_pileup_ins_counts_device(self.handle), 4 * self.n_cols * self.ins_slots * self.alphabet_len, self)

    def _letters(self, ref, lo, n):
        """``(device pointer of the letter of column lo, a DeviceArena to close or None)`` for ``n`` letters given as a host
        array or as ``(DeviceArena, offset)``."""
        if isinstance(ref, tuple):
            arena, off = ref
            if not isinstance(arena, DeviceArena) or arena.device != self.device or not 0 <= int(off) <= arena.nbytes - n:
                raise ValueError('letters are (DeviceArena on device %d, offset) with %d letters behind the offset' % (self.device, n))
            return arena.ptr + int(off), None
        letters = _as_u8(ref)
        if len(letters) != n:
            raise ValueError('%d letters for %d columns' % (len(letters), n))
        held = DeviceArena(letters if len(letters) else np.zeros(1, np.uint8), device=self.device)
        return held.ptr, held

    def add_letters(self, ref, weight=1, lo=0, stream=None):
        """The self vote (``pw_pileup_add_letters``): column ``lo + x`` gains ``weight`` in the channel of letter ``x`` of
        ``ref`` -- a host array, or ``(DeviceArena, offset)`` with ``n_cols - lo`` letters behind the offset, as for
        :meth:`call`.  A letter outside the alphabet adds nothing."""
        weight, lo = int(weight), int(lo)
        if not 0 <= weight < 1 << 32:
            raise ValueError('weight must fit 32 bits')
        if isinstance(ref, tuple):
            lo, hi = self._range(lo, None)
        else:
            lo, hi = self._range(lo, lo + len(_as_u8(ref)))
        ptr, held = self._letters(ref, lo, hi - lo)
        try:
            self._ck(self.lib.pw_pileup_add_letters(self.handle, ptr, lo, hi, weight, stream), 'pw_pileup_add_letters')
        finally:
            if held is not None:
                held.close()                 # (pw_arena_free waits for the device: the kernel has read the letters by then)

    def polish(self, ref, offs, lens, min_depth=1, stream=None, columns=False):
        """The polished reads (``pw_pileup_polish``; the rule is in include/pw_polish.h): read ``r`` has its letters and its
        columns at ``offs[r] .. offs[r] + lens[r]``; ``ref`` holds one letter per column of the pileup, a host array or
        ``(DeviceArena, offset)`` as for :meth:`call`.  Returns ``(letters uint8, offsets int64[n + 1], stats)``: read ``r``
        is ``letters[offsets[r]:offsets[r + 1]]`` and ``stats[r]`` its :data:`POLISH_STATS_DTYPE` record.  ``columns=True``
        polishes one column per lane (``pw_pileup_polish_columns``, include/pw_rounds.h): the same triple, for reads that come
        in column order and do not overlap, and :meth:`colmap` then returns the map from columns to polished letters."""
        offsets, stats, letters = self._polish(ref, offs, lens, min_depth, stream, columns, True)
        return letters, offsets, stats

    def _polish(self, ref, offs, lens, min_depth, stream, columns, fetch):
        """:meth:`polish`; ``(offsets, stats)`` without ``fetch``: the letters stay on the device (:meth:`polished_letters`)."""
        entry = 'pw_pileup_polish_columns' if columns else 'pw_pileup_polish'
        min_depth = int(min_depth)
        if not 0 <= min_depth < 1 << 32:
            raise ValueError('min_depth must fit 32 bits')
        o = np.ascontiguousarray(offs, np.int64).reshape(-1)
        ln = np.ascontiguousarray(lens, np.int32).reshape(-1)
        if len(o) != len(ln):
            raise ValueError('%d offsets for %d lengths' % (len(o), len(ln)))
        if len(o) and ((ln < 0).any() or (o < 0).any() or (o + ln.astype(np.int64) > self.n_cols).any()):
            bad = int(np.flatnonzero((ln < 0) | (o < 0) | (o + ln.astype(np.int64) > self.n_cols))[0])
            raise ValueError('read %d lies outside the pileup of %d columns' % (bad, self.n_cols))
        ptr, held = self._letters(ref, 0, self.n_cols)
        try:
            self._ck(getattr(self.lib, entry)(self.handle, ptr, o.ctypes.data, ln.ctypes.data, len(o), min_depth, stream), entry)
            offsets, stats = np.zeros(len(o) + 1, np.int64), np.zeros(len(o), POLISH_STATS_DTYPE)
            self._ck(self.lib.pw_pileup_polished_offsets(self.handle, offsets.ctypes.data), 'pw_pileup_polished_offsets')
            if fetch:
                letters = self.polished_letters()
            self._ck(self.lib.pw_pileup_polished_stats(self.handle, stats.ctypes.data), 'pw_pileup_polished_stats')
        finally:
            if held is not None:
                held.close()
        return (offsets, stats, letters) if fetch else (offsets, stats)

    def polished_letters(self):
        """The letters of the last :meth:`polish`, all reads one after another (uint8)."""
        total = int(self.lib.pw_pileup_polished_total(self.handle))
        if total < 0:
            raise RuntimeError('pw_pileup_polished_total failed: ' + W.last_error())
        letters = np.zeros(total, np.uint8)
        self._ck(self.lib.pw_pileup_polished_letters(self.handle, letters.ctypes.data), 'pw_pileup_polished_letters')
        return letters

    def colmap(self, lo=0, hi=None):
        """Entries ``[lo, hi)`` of the coordinate map of the last :meth:`polish` with ``columns=True`` (``uint64``, ``n_cols + 1``
        entries in all): ``colmap[c]`` is where the letters of column ``c`` begin among the polished letters."""
        lo = int(lo)
        hi = self.n_cols + 1 if hi is None else int(hi)
        if not 0 <= lo <= hi <= self.n_cols + 1:
            raise ValueError('entries [%d, %d) outside 0 .. %d' % (lo, hi, self.n_cols + 1))
        out = np.zeros(hi - lo, np.uint64)
        self._ck(self.lib.pw_pileup_colmap(self.handle, lo, hi, out.ctypes.data), 'pw_pileup_colmap')
        return out

    def consensus(self, lo=0, hi=None):
        """The ``call`` bytes of the columns ``[lo, hi)``: a letter, ``alphabet_len`` for a deletion, 255 for no call."""
        return self.sites(lo, hi)['call'].copy()

    def variants(self, lo=0, hi=None):
        """The column indices in ``[lo, hi)`` flagged ``PW_PILEUP_DIFFERS`` or ``PW_PILEUP_INSERT`` by the last :meth:`call`."""
        lo, hi = self._range(lo, hi)
        flags = self.sites(lo, hi)['flags']
        return lo + np.flatnonzero(flags & (W.PW_PILEUP_DIFFERS | W.PW_PILEUP_INSERT)).astype(np.int64)


class BatchAligner(object):
    """Plan, upload, solve and trace back a batch of pairs.

    Args:
        pairs: iterable of ``(origin, mutant)``; each a :class:`Sequence` or an array of letter indices.
    Keyword Args:
        alphabet_len (int): number of letters (default: from the first Sequence, else max letter + 1).
        alnmode, alntype, subst_scores, match_score, mismatch_score, go_score, ge_score: as ``Aligner``.
        diag_range: one ``(dmin, dmax)`` for all pairs or a list with one per pair (banded mode).
        device (int): HIP device ordinal.  flags (int): ``PW_FLAG_*`` of include/pw_batch.h.
        check_band (bool): apply the reference's Python-side ``diag_range`` assertion (default True).
    """

    def __init__(self, pairs, **kw):
        self.lib = W.load()
        self.alnmode = kw.get('alnmode', W.STD_MODE)
        self.alntype = kw.get('alntype', W.GLOBAL)
        pairs = list(pairs)
        self.n = len(pairs)
        L = kw.get('alphabet_len')
        seqs = []
        for (o, m) in pairs:
            if L is None and isinstance(o, Sequence):
                L = len(o.alphabet)
            seqs.append((_as_u8(o), _as_u8(m)))
        if L is None:
            L = 1 + max([0] + [int(s.max()) for p in seqs for s in p if s.size])
        self.L = L
        subst = kw.get('subst_scores')
        if subst is None:
            match, mismatch = kw.get('match_score', 1), kw.get('mismatch_score', 0)
            subst = [[match if i == j else mismatch for i in range(L)] for j in range(L)]
        assert len(subst) == L
        self.subst_scores = subst
        self.go_score, self.ge_score = kw.get('go_score', 0), kw.get('ge_score', 0)
        dr = kw.get('diag_range')
        if self.alnmode == W.BANDED_MODE:
            assert dr is not None, 'banded mode needs diag_range'
            drs = [dr] * self.n if (len(dr) == 2 and not hasattr(dr[0], '__len__')) else list(dr)
            assert len(drs) == self.n
        else:
            drs = [(0, 0)] * self.n
        # arena: every sequence on a 16-byte boundary
        offs, total = [], 0
        for (o, m) in seqs:
            oo = total
            total += (len(o) + 15) // 16 * 16 + 16
            mo = total
            total += (len(m) + 15) // 16 * 16 + 16
            offs.append((oo, mo))
        self.arena = np.zeros(max(total, 16), np.uint8)
        self._pairs = (W.pw_pair * max(self.n, 1))()
        for k, ((o, m), (oo, mo), (dmin, dmax)) in enumerate(zip(seqs, offs, drs)):
            self.arena[oo:oo + len(o)] = o
            self.arena[mo:mo + len(m)] = m
            if self.alnmode == W.BANDED_MODE and kw.get('check_band', True):
                # the reference's Python-side check (pw.py:224-226); check_band=False hands the band to
                # the C side unchecked, which clamps / rejects it like dptable_init
                assert -len(m) <= dmin <= dmax <= len(o), 'diag_range outside the table'
            self._pairs[k] = W.pw_pair(oo, mo, len(o), len(m), int(dmin), int(dmax))
        self.lens = [(len(o), len(m)) for (o, m) in seqs]
        S = np.ascontiguousarray(np.asarray(subst, dtype=np.float64).reshape(L, L))
        self._S = S
        sc = W.pw_scoring(self.alnmode, self.alntype, L, S.ctypes.data_as(C.POINTER(C.c_double)),
                          float(self.go_score), float(self.ge_score))
        self.device = kw.get('device', 0)
        self.flags = kw.get('flags', 0)
        self.handle = self.lib.pw_batch_create(self.device, C.byref(sc), self.n, self._pairs,
                                               self.arena.nbytes, self.flags)
        if not self.handle:
            raise RuntimeError('pw_batch_create failed: ' + W.last_error())
        if kw.get('upload', True):
            self.upload()

    @classmethod
    def from_arena(cls, arena, offsets, lengths, pairs, diag_ranges=None, device_arena=None, **kw):
        """Pairs that REFER to reads of one shared arena (:func:`pack_reads`) instead of carrying copies: ``pairs`` is
        an (n, 2) array of read indices (origin, mutant), ``diag_ranges`` an (n, 2) array in banded mode.  This is the
        shape of overlap pipelines, where every read takes part in dozens of pairs.  With ``device_arena`` (a
        :class:`DeviceArena` of the same arena) the batch reads the reads from that device copy -- uploaded once for
        all the batches of a job -- instead of allocating and uploading its own; ``arena_bytes`` then gives the size of that
        copy when it holds more frames than ``arena`` (:meth:`DeviceArena.with_reverse_complements`)."""
        self = cls.__new__(cls)
        self.lib = W.load()
        self.alnmode = kw.get('alnmode', W.STD_MODE)
        self.alntype = kw.get('alntype', W.GLOBAL)
        pairs = np.ascontiguousarray(pairs, np.int64).reshape(-1, 2)
        self.n = len(pairs)
        L = kw['alphabet_len']
        self.L = L
        subst = kw.get('subst_scores')
        if subst is None:
            match, mismatch = kw.get('match_score', 1), kw.get('mismatch_score', 0)
            subst = [[match if i == j else mismatch for i in range(L)] for j in range(L)]
        self.subst_scores = subst
        self.go_score, self.ge_score = kw.get('go_score', 0), kw.get('ge_score', 0)
        offsets, lengths = np.asarray(offsets, np.int64), np.asarray(lengths, np.int64)
        assert (offsets % 4 == 0).all(), 'reads must start on 4-byte boundaries'
        rec = np.zeros(max(self.n, 1), PAIR_DTYPE)
        rec['origin_off'][:self.n] = offsets[pairs[:, 0]]; rec['mutant_off'][:self.n] = offsets[pairs[:, 1]]
        rec['origin_len'][:self.n] = lengths[pairs[:, 0]]; rec['mutant_len'][:self.n] = lengths[pairs[:, 1]]
        if self.alnmode == W.BANDED_MODE:
            dr = np.asarray(diag_ranges, np.int64).reshape(-1, 2)
            assert len(dr) == self.n
            if kw.get('check_band', True):
                assert ((-rec['mutant_len'][:self.n] <= dr[:, 0]) & (dr[:, 0] <= dr[:, 1]) &
                        (dr[:, 1] <= rec['origin_len'][:self.n])).all(), 'diag_range outside the table'
            rec['dmin'][:self.n] = dr[:, 0]; rec['dmax'][:self.n] = dr[:, 1]
        self._pairs = rec
        self.arena = np.ascontiguousarray(arena, np.uint8)
        self.lens = None
        S = np.ascontiguousarray(np.asarray(subst, dtype=np.float64).reshape(L, L))
        self._S = S
        sc = W.pw_scoring(self.alnmode, self.alntype, L, S.ctypes.data_as(C.POINTER(C.c_double)),
                          float(self.go_score), float(self.ge_score))
        self.device = kw.get('device', 0)
        self.flags = kw.get('flags', 0) | (W.PW_FLAG_SHARED_ARENA if device_arena is not None else 0)
        arena_bytes = int(kw['arena_bytes']) if device_arena is not None and kw.get('arena_bytes') else self.arena.nbytes
        self.handle = self.lib.pw_batch_create(self.device, C.byref(sc), self.n, rec.ctypes.data_as(C.POINTER(W.pw_pair)),
                                               arena_bytes, self.flags)
        if not self.handle:
            raise RuntimeError('pw_batch_create failed: ' + W.last_error())
        if device_arena is not None:
            assert device_arena.device == self.device and device_arena.nbytes >= arena_bytes
            self._device_arena = device_arena          # keeps it alive as long as the batch
            self._ck(self.lib.pw_batch_share_arena(self.handle, device_arena.ptr), 'pw_batch_share_arena')
        else:
            self.upload()
        return self

    # ---- lifecycle ----
    def close(self):
        if getattr(self, 'handle', None):
            self.lib.pw_batch_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        if rc != 0:
            raise RuntimeError('%s failed: %s' % (what, W.last_error()))

    # ---- planning info ----
    @property
    def cells(self):
        """Cells the reference would allocate for the batch: the GCUPS denominator."""
        return self.lib.pw_batch_cells(self.handle)

    @property
    def algorithmic_bytes(self):
        return self.lib.pw_batch_algorithmic_bytes(self.handle)

    @property
    def score_dtype(self):
        return 'f64' if self.lib.pw_batch_score_type(self.handle) else 'i32'

    @property
    def kernel_name(self):
        return self.lib.pw_batch_kernel_name(self.handle).decode()

    def init_rc(self, k):
        return self.lib.pw_batch_init_rc(self.handle, k)

    def band(self, k):
        a, b, r = C.c_int32(), C.c_int32(), C.c_int32()
        self.lib.pw_batch_band(self.handle, k, C.byref(a), C.byref(b), C.byref(r))
        return a.value, b.value, r.value

    # ---- data movement and kernels ----
    def upload(self):
        self._ck(self.lib.pw_batch_upload_arena(self.handle, self.arena.ctypes.data, self.arena.nbytes),
                 'pw_batch_upload_arena')

    def upload_async(self, pinned, stream=None):
        """H2D of the arena from a :class:`PinnedArray` holding it, asynchronous on ``stream``."""
        self._ck(self.lib.pw_batch_upload_arena_async(self.handle, pinned.ptr, self.arena.nbytes, stream),
                 'pw_batch_upload_arena_async')

    def results_async(self, pinned, stream=None):
        """D2H of the 32-byte records into a :class:`PinnedArray` (``32 * n`` bytes), asynchronous on ``stream``."""
        self._ck(self.lib.pw_batch_results_async(self.handle, pinned.ptr, stream), 'pw_batch_results_async')

    def transcripts_async(self, pinned, stream=None):
        """D2H of all transcript slots into a :class:`PinnedArray` (``transcripts_bytes`` bytes), asynchronous."""
        self._ck(self.lib.pw_batch_transcripts_async(self.handle, pinned.ptr, stream), 'pw_batch_transcripts_async')

    @property
    def transcripts_bytes(self):
        return int(self.lib.pw_batch_transcripts_bytes(self.handle))

    def solve(self, stream=None):
        self._ck(self.lib.pw_batch_solve(self.handle, stream), 'pw_batch_solve')

    def traceback(self, stream=None):
        self._ck(self.lib.pw_batch_traceback(self.handle, stream), 'pw_batch_traceback')

    def traceback_from(self, ends, stream=None):
        e = np.ascontiguousarray(np.asarray(ends, dtype=np.int32).reshape(self.n, 2))
        self._ck(self.lib.pw_batch_traceback_from(self.handle, e.ctypes.data_as(C.POINTER(C.c_int32)), stream),
                 'pw_batch_traceback_from')

    def sync(self, stream=None):
        self._ck(self.lib.pw_batch_sync(self.handle, stream), 'pw_batch_sync')

    def run(self, stream=None):
        """solve + traceback + sync; returns ``results()``."""
        self.solve(stream)
        self.traceback(stream)
        self.sync(stream)
        return self.results()

    # ---- results ----
    def results(self):
        """Structured array (RESULT_DTYPE), one record per pair (synchronous D2H)."""
        out = np.zeros(max(self.n, 1), RESULT_DTYPE)
        self._ck(self.lib.pw_batch_results(self.handle, out.ctypes.data), 'pw_batch_results')
        return out[:self.n]

    def transcripts(self, results=None, slots=None):
        """List with one transcript string (or None) per pair (synchronous D2H, unless ``slots`` already holds the
        slot buffer, e.g. from :meth:`transcripts_async`)."""
        res = self.results() if results is None else results
        nb = self.lib.pw_batch_transcripts_bytes(self.handle)
        if slots is not None:
            buf = slots
        else:
            buf = np.zeros(max(nb, 1), np.uint8)
            self._ck(self.lib.pw_batch_transcripts(self.handle, buf.ctypes.data), 'pw_batch_transcripts')
        out = []
        off, cap = C.c_uint64(), C.c_int32()
        for k in range(self.n):
            n = int(res['tx_len'][k])
            if n <= 0:
                out.append(None)
                continue
            self.lib.pw_batch_tx_slot(self.handle, k, C.byref(off), C.byref(cap))
            end = off.value + cap.value
            out.append(buf[end - n:end].tobytes().decode('ascii'))
        return out

    def transcript_slots(self):
        """(offsets, capacities) of all transcript slots as arrays (ops of pair k END at offset + capacity)."""
        off, cap = np.zeros(self.n, np.uint64), np.zeros(self.n, np.int32)
        o, c = C.c_uint64(), C.c_int32()
        for k in range(self.n):
            self.lib.pw_batch_tx_slot(self.handle, k, C.byref(o), C.byref(c))
            off[k], cap[k] = o.value, c.value
        return off, cap

    # ---- compacted transcripts (what a gather should move) ----
    def pack_transcripts(self, stream=None):
        """After a traceback on ``stream``: the ops of all pairs back to back in pair order and their exclusive offsets
        (uint64[n + 1]), device-resident (``pw_batch_pack_transcripts``).  Asynchronous on ``stream``."""
        self._ck(self.lib.pw_batch_pack_transcripts(self.handle, stream), 'pw_batch_pack_transcripts')

    def packed_device(self):
        """(packed bytes, offsets) as :class:`DeviceBuffer` views; the packed view spans the whole buffer (its first
        ``offsets[n]`` bytes are the ops)."""
        return (DeviceBuffer(self.lib.pw_batch_packed_device(self.handle), max(self.transcripts_bytes, 16), self),
                DeviceBuffer(self.lib.pw_batch_packed_offsets_device(self.handle), 8 * (self.n + 1), self))

    def packed_total_async(self, pinned, stream=None):
        """D2H of the total number of packed bytes into a :class:`PinnedArray` of 8 bytes, ordered on ``stream``."""
        self._ck(self.lib.pw_batch_packed_total_async(self.handle, pinned.ptr, stream), 'pw_batch_packed_total_async')

    def packed(self):
        """(bytes uint8[total], offsets uint64[n + 1]) on the host (synchronous)."""
        off = np.zeros(self.n + 1, np.uint64)
        self._ck(self.lib.pw_batch_packed(self.handle, None, 0, off.ctypes.data), 'pw_batch_packed')
        buf = np.zeros(max(int(off[-1]), 1), np.uint8)
        self._ck(self.lib.pw_batch_packed(self.handle, buf.ctypes.data, buf.nbytes, None), 'pw_batch_packed')
        return buf[:int(off[-1])], off

    @staticmethod
    def transcripts_from_packed(buf, offsets):
        """List of transcript strings (None for pairs without one) from a packed buffer and its offsets."""
        offsets = np.asarray(offsets, np.int64)
        raw = np.asarray(buf, np.uint8).tobytes()
        return [raw[offsets[k]:offsets[k + 1]].decode('ascii') if offsets[k + 1] > offsets[k] else None
                for k in range(len(offsets) - 1)]

    # ---- alignment summaries (include/pw_txsum.h): the transcripts reduced where they are ----
    def summarize(self, stream=None):
        """After a traceback on ``stream``: one :data:`SUMMARY_DTYPE` record per pair -- op counts, gap runs, first / last
        match and the letters in front of and behind them -- reduced from the ops on the device (``pw_batch_summarize``).
        Asynchronous on ``stream``.  The records describe the traceback in front of the call: after another traceback
        they are stale until ``summarize`` runs again (:meth:`summaries` does that itself)."""
        self._ck(self.lib.pw_batch_summarize(self.handle, stream), 'pw_batch_summarize')

    def summaries(self):
        """Structured array (SUMMARY_DTYPE), one record per pair (synchronous D2H; runs the kernel first when a traceback
        has happened since the last :meth:`summarize`).  ``flags`` is 0, both match indices -1 and every count 0 for a
        pair without a transcript."""
        out = np.zeros(max(self.n, 1), SUMMARY_DTYPE)
        self._ck(self.lib.pw_batch_summaries(self.handle, out.ctypes.data), 'pw_batch_summaries')
        return out[:self.n]

    def summaries_async(self, pinned, stream=None):
        """D2H of the 48-byte summaries into a :class:`PinnedArray` (``48 * n`` bytes), asynchronous on ``stream``, behind a
        :meth:`summarize` on it."""
        self._ck(self.lib.pw_batch_summaries_async(self.handle, pinned.ptr, stream), 'pw_batch_summaries_async')

    def summaries_device(self):
        return DeviceBuffer(self.lib.pw_batch_summaries_device(self.handle), 48 * self.n, self)

    # ---- CIGARs (include/pw_cigar.h): the transcripts run-length encoded where they are ----
    def cigars(self, form='extended', stream=None):
        """After a traceback on ``stream``: ``(runs uint32[total], offsets uint64[n + 1])`` on the host -- the runs
        ``(length << 4) | op`` of all pairs back to back in transcript order, pair ``k`` owning
        ``runs[offsets[k]:offsets[k + 1]]`` (``pw_batch_cigars``, then a synchronous D2H).  ``form`` is ``'extended'`` (``=`` /
        ``X``) or ``'classic'`` (``M``).  A pair without a summary (:meth:`summaries`) has zero runs.  The call reads the
        8-byte total back between the offsets and the write kernel: it blocks on ``stream`` once."""
        f = _cigar_form(form)
        self._ck(self.lib.pw_batch_cigars(self.handle, f, stream), 'pw_batch_cigars')
        if stream is not None:
            self.sync(stream)
        off = np.zeros(self.n + 1, np.uint64)
        self._ck(self.lib.pw_batch_cigar(self.handle, f, None, 0, off.ctypes.data), 'pw_batch_cigar')
        total = int(off[-1])
        runs = np.zeros(max(total, 1), np.uint32)
        self._ck(self.lib.pw_batch_cigar(self.handle, f, runs.ctypes.data, runs.size, None), 'pw_batch_cigar')
        return runs[:total], off

    def cigars_device(self):
        """(runs, offsets) of the last ``pw_batch_cigars`` -- :meth:`cigars`, or a direct call -- as :class:`DeviceBuffer` views;
        the runs view spans ``pw_batch_cigar_total`` runs."""
        runs, off = self.lib.pw_batch_cigar_runs_device(self.handle), self.lib.pw_batch_cigar_offsets_device(self.handle)
        if not runs or not off:
            raise RuntimeError('cigars_device before cigars')
        return DeviceBuffer(runs, 4 * int(self.lib.pw_batch_cigar_total(self.handle)), self), DeviceBuffer(off, 8 * (self.n + 1), self)

    # ---- pileups (include/pw_pileup.h): the transcripts scattered into per-column counts where they are ----
    def pileup_add(self, pileup, col0=None, arena_first=0, stream=None, sides='origin', mutant_col0=None, reverse=None, complement=None):
        """After a traceback on ``stream``: every pair with an alignment adds its ops to the columns of its origin in
        ``pileup`` (a :class:`Pileup` on the same device; ``pw_batch_pileup_add``, asynchronous on ``stream``).  The origin
        frame of pair ``k`` starts at column ``col0[k]`` -- an int64 per pair, negative to skip the pair -- or, without
        ``col0``, at its arena offset minus ``arena_first``; a pair whose frame does not lie inside the pileup adds nothing.
        Adding is cumulative.

        ``sides``: ``'origin'`` (with the other defaults and a pileup without an insertion plane: the call above, exactly), ``'mutant'`` or ``'both'``
        (``pw_batch_pileup_add_sides``, include/pw_polish.h): the mutant side adds the swapped pair to the columns of the
        mutant, whose frame starts at ``mutant_col0[k]`` or at its arena offset minus ``arena_first``; where ``reverse[k]`` is
        set the mutant frame is read backwards through ``complement`` (a table of ``alphabet_len`` letters), so that the
        columns are the forward letters of a read whose reverse complement was aligned.  These calls also fill the
        insertion plane of a pileup that has one."""
        if sides not in _SIDES:
            raise ValueError("sides is 'origin', 'mutant' or 'both', not %r" % (sides,))

        def per_pair(a, dtype, what):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype).reshape(-1)
            if len(a) != self.n:
                raise ValueError('%s has %d entries for %d pairs' % (what, len(a), self.n))
            return a
        c, mc = per_pair(col0, np.int64, 'col0'), per_pair(mutant_col0, np.int64, 'mutant_col0')
        rv = per_pair(None if reverse is None else np.asarray(reverse) != 0, np.uint8, 'reverse')
        comp = None
        if rv is not None and rv.any():
            if sides == 'origin':
                raise ValueError("reverse applies to the mutant side: sides is 'mutant' or 'both'")
            if complement is None:
                raise ValueError('reversed pairs need a complement table')
            comp = np.ascontiguousarray(complement, np.uint8).reshape(-1)
        if not isinstance(pileup, Pileup) or not pileup.handle:
            raise ValueError('pileup must be an open Pileup')
        if sides == 'origin' and mc is None and rv is None and complement is None and not pileup.ins_slots:
            self._ck(self.lib.pw_batch_pileup_add(self.handle, pileup.handle, None if c is None else c.ctypes.data, int(arena_first), stream),
                     'pw_batch_pileup_add')
            return

        def ptr(a):
            return None if a is None else a.ctypes.data
        self._ck(self.lib.pw_batch_pileup_add_sides(self.handle, pileup.handle, _SIDES[sides], ptr(c), ptr(mc), ptr(rv), ptr(comp),
                                                    0 if comp is None else len(comp), int(arena_first), stream),
                 'pw_batch_pileup_add_sides')

    def scores_plane(self, k):
        """Score of every cell of pair k as ``plane[d - dmin, a]`` (needs PW_FLAG_DUMP_SCORES)."""
        X, Y = self.lens[k]
        dmin, dmax, _ = self.band(k)
        nd, pitch = dmax - dmin + 1, min(X, Y) + 1
        out = np.zeros(nd * pitch, np.float64)
        self._ck(self.lib.pw_batch_scores(self.handle, k, out.ctypes.data_as(C.POINTER(C.c_double)), out.size),
                 'pw_batch_scores')
        return out.reshape(nd, pitch)

    def masks(self, k):
        """Tie mask of every in-table cell of pair k (bits B 1, D 2, I 4, M 8), flat in the reference's table order: standard
        mode ``[x * (Y + 1) + y]``, banded mode rows ``d - dmin`` back to back (``pw_batch_masks``).  The packed 16-bit
        kernels and the strips store no M bit."""
        out = np.zeros(max(int(self.lib.pw_batch_pair_cells(self.handle, k)), 1), np.uint8)
        self._ck(self.lib.pw_batch_masks(self.handle, k, out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size),
                 'pw_batch_masks')
        return out

    def results_device(self):
        return DeviceBuffer(self.lib.pw_batch_results_device(self.handle), 32 * self.n, self)

    def transcripts_device(self):
        return DeviceBuffer(self.lib.pw_batch_transcripts_device(self.handle),
                            self.lib.pw_batch_transcripts_bytes(self.handle), self)

    def fill_ms(self):
        return float(self.lib.pw_batch_fill_ms(self.handle))

    def trace_ms(self):
        return float(self.lib.pw_batch_trace_ms(self.handle))


def align_batch(pairs, **kw):
    """One-call convenience: returns ``(results, transcripts)`` for the pairs."""
    with BatchAligner(pairs, **kw) as b:
        res = b.run()
        return res, b.transcripts(res)


def summary_dict(rec):
    """One SUMMARY_DTYPE record as a dict of Python ints."""
    return {f: int(rec[f]) for f in SUMMARY_DTYPE.names}


def summarize_transcripts(transcripts, device=0):
    """Summaries (SUMMARY_DTYPE, one record per transcript) of transcripts that are not in a batch's slots, through the
    same device routine (``pw_tx_summarize_packed``): ``transcripts`` is a list of ``str`` / ``None``, or ``(buf, offsets)``
    as :meth:`BatchAligner.packed` returns them.  ``None`` and ``''`` get the record of a pair without a transcript."""
    if isinstance(transcripts, tuple) and len(transcripts) == 2 and isinstance(transcripts[0], np.ndarray):
        buf = np.ascontiguousarray(transcripts[0], np.uint8)
        off = np.ascontiguousarray(transcripts[1], np.uint64)
        assert off.ndim == 1 and off.size >= 1 and int(off[-1]) <= buf.size
    else:
        raw = [(t or '').encode('ascii') for t in transcripts]
        off = np.zeros(len(raw) + 1, np.uint64)
        if raw:
            off[1:] = np.cumsum([len(r) for r in raw])
        buf = np.frombuffer(b''.join(raw), np.uint8)
    n = off.size - 1
    out = np.zeros(max(n, 1), SUMMARY_DTYPE)
    if W.load().pw_tx_summarize_packed(device, buf.ctypes.data if buf.size else None, off.ctypes.data, n, out.ctypes.data) != 0:
        raise RuntimeError('pw_tx_summarize_packed failed: ' + W.last_error())
    return out[:n]


def _packed_transcripts(transcripts):
    """``(buf uint8, offsets uint64[n + 1])`` of a list of ``str`` / ``None``, or of such a tuple itself."""
    if isinstance(transcripts, tuple) and len(transcripts) == 2 and isinstance(transcripts[0], np.ndarray):
        buf = np.ascontiguousarray(transcripts[0], np.uint8)
        off = np.ascontiguousarray(transcripts[1], np.uint64)
        assert off.ndim == 1 and off.size >= 1 and int(off[-1]) <= buf.size
        return buf, off
    raw = [(t or '').encode('ascii') for t in transcripts]
    off = np.zeros(len(raw) + 1, np.uint64)
    if raw:
        off[1:] = np.cumsum([len(r) for r in raw])
    return np.frombuffer(b''.join(raw), np.uint8), off


def cigars_of_transcripts(transcripts, form='extended', device=0):
    """``(runs uint32[total], offsets uint64[n + 1])`` of transcripts that are not in a batch's slots, through the same
    device routine (``pw_tx_cigar_packed``): ``transcripts`` is a list of ``str`` / ``None``, or ``(buf, offsets)`` as
    :meth:`BatchAligner.packed` returns them.  ``None`` and ``''`` have zero runs."""
    f = _cigar_form(form)
    buf, off = _packed_transcripts(transcripts)
    n = off.size - 1
    lib = W.load()
    roff = np.zeros(n + 1, np.uint64)
    ops = buf.ctypes.data if buf.size else None
    runs = np.zeros(max(int(off[-1]) - int(off[0]), 1), np.uint32)       # (room for one run per op: one call, no size query)
    if lib.pw_tx_cigar_packed(device, ops, off.ctypes.data, n, f, runs.ctypes.data, runs.size, roff.ctypes.data) != 0:
        raise RuntimeError('pw_tx_cigar_packed failed: ' + W.last_error())
    return runs[:int(roff[-1])].copy(), roff


def cigar_strings(runs, offsets):
    """One CIGAR string per pair from ``(runs, offsets)`` of :meth:`BatchAligner.cigars`; zero runs give ``''``."""
    runs, offsets = np.asarray(runs, np.uint32), np.asarray(offsets, np.int64)
    lens, ops = (runs >> 4).tolist(), (runs & 15).tolist()
    return [''.join('%d%s' % (lens[r], CIGAR_OPS[ops[r]]) for r in range(int(offsets[k]), int(offsets[k + 1])))
            for k in range(len(offsets) - 1)]


def cigar_of_transcript(tx, form='extended'):
    """The CIGAR string of one transcript over ``MSID``, on the host (``None`` and ``''`` give ``''``)."""
    letters = _CIGAR_LETTERS[_cigar_form(form)]
    out, cur, n = [], None, 0
    for op in tx or '':
        if op not in letters:
            raise ValueError('transcript op %r is none of M, S, I, D' % (op,))
        if letters[op] == cur:
            n += 1
            continue
        if cur is not None:
            out.append('%d%s' % (n, cur))
        cur, n = letters[op], 1
    if cur is not None:
        out.append('%d%s' % (n, cur))
    return ''.join(out)


def transcript_of_cigar(s):
    """The transcript of a CIGAR string in the extended form.  ``ValueError`` for a classic ``M`` (it does not say which of
    its letters match), any other op and anything that is not a CIGAR."""
    import re
    if not re.fullmatch(r'(?:[0-9]+[A-Za-z=])*', s):
        raise ValueError('not a CIGAR string: %r' % (s,))
    back = {'=': 'M', 'X': 'S', 'I': 'I', 'D': 'D'}
    out = []
    for n, op in re.findall(r'([0-9]+)([A-Za-z=])', s):
        if op not in back:
            raise ValueError('CIGAR op %r has no transcript letter (only the extended form =, X, I, D has)' % (op,))
        out.append(back[op] * int(n))
    return ''.join(out)


def plan_only(shapes, alnmode=W.STD_MODE, alntype=W.GLOBAL, alphabet_len=4, subst_scores=None, match_score=1, mismatch_score=0,
              go_score=0, ge_score=0, flags=0, ramp_free=False, stamp_group=False, lds_feed=False, pair_keys=False,
              lds_exchange=False):
    """What :class:`BatchAligner` would choose for problems of these shapes, without a GPU and without allocating anything
    (``pw_plan_only``): ``shapes`` is a list of ``(origin_len, mutant_len)`` or ``(origin_len, mutant_len, dmin, dmax)``.
    Returns a dict: ``kernel`` (as :attr:`BatchAligner.kernel_name`), ``score_dtype``, ``scale_shift`` (dyadic scaling:
    scores held times ``2**shift``), the number of pairs on one-wavefront kernels / workgroup kernels / the tiled kernel /
    the strip pipeline, ``packed_rule`` (-1 unless a packed 16-bit kernel), ``matrix`` (packed kernel in matrix form) and, asked for
    with ``ramp_free=True``, ``ramp_free`` (the packed kernel runs its start and end blocks on the steady body;
    ``PWLIB_RAMP_BLOCKS=1`` turns that off) and, asked for with ``stamp_group=True``, ``stamp_group`` (4: the packed kernel
    stamps its running best once per four blocks, the grouped kernel; 1 otherwise and under ``PWLIB_STAMP_GROUP=1``) and,
    asked for with ``lds_feed=True``, ``lds_feed`` (the grouped kernel reads its letters from LDS; ``PWLIB_LDS_FEED=0`` turns
    that off) and, asked for with ``pair_keys=True``, ``pair_keys`` (that kernel keeps one running-best key per two cells;
    ``PWLIB_PAIR_KEYS=0`` turns that off) and, asked for with ``lds_exchange=True``, ``lds_exchange`` (that kernel hands its
    lane-crossing offers on through LDS; ``PWLIB_LDS_EXCHANGE=0`` turns that off)."""
    lib = W.load()
    L = alphabet_len
    if subst_scores is None:
        subst_scores = [[match_score if i == j else mismatch_score for i in range(L)] for j in range(L)]
    S = np.ascontiguousarray(np.asarray(subst_scores, dtype=np.float64).reshape(L, L))
    sc = W.pw_scoring(alnmode, alntype, L, S.ctypes.data_as(C.POINTER(C.c_double)), float(go_score), float(ge_score))
    pairs = (W.pw_pair * max(len(shapes), 1))()
    off = 0
    for k, sh in enumerate(shapes):
        X, Y = int(sh[0]), int(sh[1])
        dmin, dmax = (int(sh[2]), int(sh[3])) if len(sh) > 2 else (0, 0)
        oo = off
        off += (X + 15) // 16 * 16 + 16
        mo = off
        off += (Y + 15) // 16 * 16 + 16
        pairs[k] = W.pw_pair(oo, mo, X, Y, dmin, dmax)
    name = C.create_string_buffer(128)
    info = (C.c_int32 * 8)()
    if lib.pw_plan_only(C.byref(sc), len(shapes), pairs, max(off, 16), flags, name, 128, info) != 0:
        raise RuntimeError('pw_plan_only failed: ' + W.last_error())
    out = dict(kernel=name.value.decode(), score_dtype='f64' if info[0] else 'i32', scale_shift=info[1], one_wavefront=info[2],
                workgroup=info[3], tiled=info[4], strips=info[5], packed_rule=info[6], matrix=bool(info[7] & 1))
    if ramp_free:
        out['ramp_free'] = bool(info[7] & 2)
    if stamp_group:
        out['stamp_group'] = 4 if info[7] & 4 else 1
    if lds_feed:
        out['lds_feed'] = bool(info[7] & 8)
    if pair_keys:
        out['pair_keys'] = bool(info[7] & 16)
    if lds_exchange:
        out['lds_exchange'] = bool(info[7] & 32)
    return out
