"""The overlap graph on the device (include/pw_graph.h holds the contract): overlap records, their containment / dovetail
classes, arcs, transitive reduction, unitigs and contig letters -- and the consensus stage on top of it
(include/pw_consensus.h): where every read lies on its contig, the read-against-contig alignment tasks and the polished
contigs.  Every computing call goes to the kernels of ``pw_graph.hip``, ``pw_consensus.hip`` and ``pw_rounds.hip`` (the later rounds of
the consensus, include/pw_rounds.h); there is no host fallback."""
import ctypes as C

import numpy as np

from . import _pwlib as W
from .batch import BatchAligner, DeviceArena, _as_u8, pack_reads

OVERLAP_DTYPE = np.dtype([(f, '<i4') for f in ('a', 'b', 'strand', 'cls', 'a_beg', 'a_end', 'b_beg', 'b_end', 'n_match', 'n_ops')])
ARC_DTYPE = np.dtype([(f, '<i4') for f in ('v', 'w', 'len', 'ol', 'src', 'flags')])
UNITIG_DTYPE = np.dtype([('first_member', '<i8'), ('length', '<i8'), ('n_members', '<i4'), ('head', '<i4'), ('circular', '<i4'),
                         ('pad_', '<i4')])
MEMBER_DTYPE = np.dtype([('vertex', '<i4'), ('advance', '<i4'), ('offset', '<i8')])
assert (OVERLAP_DTYPE.itemsize, ARC_DTYPE.itemsize, UNITIG_DTYPE.itemsize, MEMBER_DTYPE.itemsize) == (40, 24, 32, 16)
PLACE_DTYPE = np.dtype([('unitig', '<i4'), ('rev', '<i4'), ('pos', '<i8'), ('root', '<i4'), ('depth', '<i4')])
TASK_DTYPE = np.dtype([('col0', '<i8'), ('mut_off', '<i8')] + [(f, '<i4') for f in ('read', 'win_len', 'dmin', 'dmax', 'rev', 'pad_')])
assert (PLACE_DTYPE.itemsize, TASK_DTYPE.itemsize) == (24, 40)
NONE, WEAK, INTERNAL, A_CONTAINED, B_CONTAINED, A_TO_B, B_TO_A = range(7)
CLASS_NAMES = ('NONE', 'WEAK', 'INTERNAL', 'A_CONTAINED', 'B_CONTAINED', 'A_TO_B', 'B_TO_A')
ARC_REDUCED, ARC_REMOVED, ARC_CHAIN, ARC_DROPPED = W.PW_ARC_REDUCED, W.PW_ARC_REMOVED, W.PW_ARC_CHAIN, W.PW_ARC_DROPPED


def overlap_records(rows):
    """An :data:`OVERLAP_DTYPE` array from rows ``(a, b, strand, a_beg, a_end, b_beg, b_end, n_match, n_ops)``; ``cls`` is 0."""
    out = np.zeros(len(rows), OVERLAP_DTYPE)
    for k, row in enumerate(rows):
        (out['a'][k], out['b'][k], out['strand'][k], out['a_beg'][k], out['a_end'][k], out['b_beg'][k], out['b_end'][k],
         out['n_match'][k], out['n_ops'][k]) = row
    return out


class OverlapGraph(object):
    """The overlap graph of ``len(read_lens)`` reads, device-resident: records come from :meth:`add` (planted, host) or
    :meth:`add_batch` (a traced-back :class:`BatchAligner`), :meth:`build` classifies them, reduces the graph and lays out the
    unitigs, :meth:`contigs` writes the letters.  A context manager that frees itself, like :class:`biseqt_amd.batch.Pileup`."""

    def __init__(self, read_lens, device=0):
        self.handle = None
        lens = np.ascontiguousarray(read_lens, np.int64).reshape(-1)
        if len(lens) and (lens.min() < 0 or lens.max() >= 1 << 31):
            raise ValueError('read lengths must lie in 0 .. 2**31 - 1')
        self.read_lens = lens.astype(np.int32)
        self.n_reads, self.device = len(lens), device
        self.lib = W.load()
        self.handle = self.lib.pw_graph_create(device, self.n_reads, self.read_lens.ctypes.data)
        if not self.handle:
            raise RuntimeError('pw_graph_create failed: ' + W.last_error())

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.pw_graph_free(self.handle)
            self.handle = None

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

    def _count(self, what):
        n = int(getattr(self.lib, what)(self.handle))
        if n < 0:
            raise RuntimeError('%s failed: %s' % (what, W.last_error()))
        return n

    def __len__(self):
        return int(self.lib.pw_graph_num_overlaps(self.handle))

    @property
    def device_bytes(self):
        return int(self.lib.pw_graph_device_bytes(self.handle))

    @property
    def reduce_ms(self):
        """Device time of the reduction kernel in the last build, ms; -1 before a build and for a graph without arcs."""
        return float(self.lib.pw_graph_reduce_ms(self.handle))

    def add(self, records):
        """Append planted records: an :data:`OVERLAP_DTYPE` array (``cls`` is ignored; ``n_ops == 0`` is a pair without an
        alignment), or rows for :func:`overlap_records`."""
        recs = records if isinstance(records, np.ndarray) and records.dtype == OVERLAP_DTYPE else overlap_records(list(records))
        recs = np.ascontiguousarray(recs)
        self._ck(self.lib.pw_graph_add_overlaps(self.handle, recs.ctypes.data, len(recs)), 'pw_graph_add_overlaps')

    def add_batch(self, batch, read_a, read_b, strands=None, stream=None):
        """One record per pair of a traced-back ``batch`` (asynchronous on ``stream``): pair ``k`` aligns the whole of read
        ``read_a[k]`` with the whole of read ``read_b[k]``, or with its reverse complement where ``strands[k]`` is set."""
        if not isinstance(batch, BatchAligner) or not batch.handle:
            raise ValueError('batch must be an open BatchAligner')
        a = np.ascontiguousarray(read_a, np.int32).reshape(-1)
        b = np.ascontiguousarray(read_b, np.int32).reshape(-1)
        s = None if strands is None else np.ascontiguousarray(strands, np.uint8).reshape(-1)
        if len(a) != batch.n or len(b) != batch.n or (s is not None and len(s) != batch.n):
            raise ValueError('read_a, read_b and strands need one entry per pair of the batch (%d)' % batch.n)
        self._ck(self.lib.pw_batch_graph_add(batch.handle, self.handle, a.ctypes.data, b.ctypes.data, None if s is None else s.ctypes.data,
                                             stream), 'pw_batch_graph_add')

    def build(self, max_hang=1000, int_frac=.8, min_overlap=0, min_identity=0., fuzz=10, stream=None, max_tip_reads=0,
              max_bubble_reads=0, clean_rounds=1):
        """Classify, reduce and lay out what has been added (``pw_graph_build``; synchronous).  A second build replaces the first.
        ``max_tip_reads`` / ``max_bubble_reads`` above 0 switch on the CLEANING of include/pw_graph.h (``pw_graph_build_clean``):
        ``clean_rounds`` rounds (0 .. 8) that drop tips of at most so many reads and the weaker of parallel paths of at most so
        many reads, between the reduction and the unitigs; :meth:`dropped` tells which reads went."""
        for name, v in (('max_hang', max_hang), ('min_overlap', min_overlap), ('fuzz', fuzz)):
            if not 0 <= int(v) < 1 << 31:
                raise ValueError('%s must lie in 0 .. 2**31 - 1' % name)
        if not (np.isfinite(int_frac) and np.isfinite(min_identity)):
            raise ValueError('int_frac and min_identity must be finite')
        p = W.pw_graph_params(int(max_hang), int(min_overlap), int(fuzz), 0, float(int_frac), float(min_identity))
        for name, v in (('max_tip_reads', max_tip_reads), ('max_bubble_reads', max_bubble_reads)):
            if not 0 <= int(v) < 1 << 31:
                raise ValueError('%s must lie in 0 .. 2**31 - 1' % name)
        if not 0 <= int(clean_rounds) <= 8:
            raise ValueError('clean_rounds must lie in 0 .. 8')
        if not (int(max_tip_reads) or int(max_bubble_reads)):
            self._ck(self.lib.pw_graph_build(self.handle, C.byref(p), stream), 'pw_graph_build')
            return
        c = W.pw_graph_clean_params(int(max_tip_reads), int(max_bubble_reads), int(clean_rounds), 0)
        self._ck(self.lib.pw_graph_build_clean(self.handle, C.byref(p), C.byref(c), stream), 'pw_graph_build_clean')

    def _fetch(self, what, n, dtype):
        out = np.zeros(n, dtype)
        self._ck(getattr(self.lib, what)(self.handle, out.ctypes.data), what)
        return out

    def overlaps(self):
        """The records (:data:`OVERLAP_DTYPE`), ``cls`` as the last :meth:`build` left it."""
        return self._fetch('pw_graph_overlaps', len(self), OVERLAP_DTYPE)

    def contained(self):
        """One byte per read: 1 where some record classifies the read as contained."""
        return self._fetch('pw_graph_contained', self.n_reads, np.uint8)

    def dropped(self):
        """One byte per read: 1 where the cleaning of the last :meth:`build` dropped the read as a tip, 2 as a bubble."""
        return self._fetch('pw_graph_dropped', self.n_reads, np.uint8)

    def arcs(self):
        """``(arcs, rows)``: the sorted arc table (:data:`ARC_DTYPE`) and its row index ``int64[2 * n_reads + 1]``."""
        return self._fetch('pw_graph_arcs', self._count('pw_graph_num_arcs'), ARC_DTYPE), \
            self._fetch('pw_graph_rows', 2 * self.n_reads + 1, np.int64)

    def unitigs(self):
        """``(unitigs, members)``: :data:`UNITIG_DTYPE` records and the :data:`MEMBER_DTYPE` records they index."""
        return self._fetch('pw_graph_unitigs', self._count('pw_graph_num_unitigs'), UNITIG_DTYPE), \
            self._fetch('pw_graph_members', self._count('pw_graph_num_members'), MEMBER_DTYPE)

    def contigs(self, reads, complement=None, stream=None):
        """The contig letters of the last build, a list of uint8 arrays in unitig order.  ``reads``: the reads themselves, or
        ``(DeviceArena, offs)`` for letters that are on the device already (``offs[r]``: where read ``r`` starts).
        ``complement``: the table that turns a letter into its complement; required as soon as a member is an odd vertex."""
        n_unitigs = self._count('pw_graph_num_unitigs')     # (raises before the first build)
        arena, offs, held = self._device_reads(reads)
        comp = None if complement is None else np.ascontiguousarray(complement, np.uint8).reshape(-1)
        if comp is not None and not 1 <= len(comp) <= 256:
            raise ValueError('complement must hold 1 .. 256 letters')
        try:
            if comp is None and (self.unitigs()[1]['vertex'] & 1).any():
                raise ValueError('a member is a reverse-complemented read: contigs needs the complement table')
            self._ck(self.lib.pw_graph_contigs(self.handle, arena.ptr, offs.ctypes.data, None if comp is None else comp.ctypes.data,
                                               0 if comp is None else len(comp), stream), 'pw_graph_contigs')
            letters = self._fetch('pw_graph_contig_letters', self._count('pw_graph_contig_total'), np.uint8)
            coff = self._fetch('pw_graph_contig_offsets', n_unitigs + 1, np.int64)
        finally:
            if held is not None:
                held.close()
        return [letters[coff[u]:coff[u + 1]].copy() for u in range(n_unitigs)]

    # ---- the consensus stage (include/pw_consensus.h) ----
    def placements(self, stream=None):
        """One :data:`PLACE_DTYPE` record per read: where the read lies on the contigs of the last build (``pw_graph_place``;
        synchronous).  ``unitig == -1``: the read is unplaced."""
        self._count('pw_graph_num_unitigs')                 # (raises before the first build)
        if not self.lib.pw_graph_placements_device(self.handle):       # (not placed since the build)
            self._ck(self.lib.pw_graph_place(self.handle, stream), 'pw_graph_place')
        return self._fetch('pw_graph_placements', self.n_reads, PLACE_DTYPE)

    def _device_reads(self, reads):
        """``(arena, offs, held)``: the reads on the device, from the reads themselves (``held`` is then the arena to close) or
        from ``(DeviceArena, offs)``."""
        if isinstance(reads, tuple):
            arena, offs = reads
            offs = np.ascontiguousarray(offs, np.int64).reshape(-1)
            if not isinstance(arena, DeviceArena) or arena.device != self.device or len(offs) != self.n_reads or \
                    (len(offs) and (offs.min() < 0 or (offs + self.read_lens).max() > arena.nbytes)):
                raise ValueError('reads are (DeviceArena on device %d, offs) with every read inside the arena' % self.device)
            return arena, offs, None
        if len(reads) != self.n_reads or any(len(_as_u8(r)) != n for r, n in zip(reads, self.read_lens.tolist())):
            raise ValueError('reads must be the %d reads of the graph, with its lengths' % self.n_reads)
        host, offs, _ = pack_reads(reads)
        arena = DeviceArena(host, self.device)
        return arena, offs, arena

    def consensus_layout(self, reads, complement=None, slack=50, drift=.1, stream=None):
        """``(cstart, tasks, arena)`` of ``pw_graph_consensus_layout`` (synchronous): the padded contig starts
        ``int64[n_unitigs + 1]``, the :data:`TASK_DTYPE` records and the consensus arena as a :class:`DeviceArena` that owns
        nothing -- it is the graph's, and good until the next layout, build or :meth:`close`.  ``reads`` and ``complement``
        as for :meth:`contigs`."""
        n_unitigs = self._count('pw_graph_num_unitigs')     # (raises before the first build)
        if not 0 <= int(slack) < 1 << 31:
            raise ValueError('slack must lie in 0 .. 2**31 - 1')
        if not (np.isfinite(drift) and 0 <= drift <= 1 << 20):
            raise ValueError('drift must be finite and lie in 0 .. 2**20')
        comp = None if complement is None else np.ascontiguousarray(complement, np.uint8).reshape(-1)
        if comp is not None and not 1 <= len(comp) <= 256:
            raise ValueError('complement must hold 1 .. 256 letters')
        if comp is None and (self.unitigs()[1]['vertex'] & 1).any():
            raise ValueError('a member is a reverse-complemented read: the consensus needs the complement table')
        src, offs, held = self._device_reads(reads)
        try:
            self._ck(self.lib.pw_graph_consensus_layout(self.handle, src.ptr, offs.ctypes.data, None if comp is None else comp.ctypes.data,
                                                        0 if comp is None else len(comp), int(slack), float(drift), stream),
                     'pw_graph_consensus_layout')
        finally:
            if held is not None:
                held.close()
        return self._layout_results(n_unitigs, comp)

    def _layout_results(self, n_unitigs, comp):
        cstart = self._fetch('pw_graph_cons_cstart', n_unitigs + 1, np.int64)
        tasks = self._fetch('pw_graph_cons_tasks', self._count('pw_graph_cons_num_tasks'), TASK_DTYPE)
        if comp is None and len(tasks) and tasks['rev'].any():
            raise ValueError('a read lies reverse-complemented on its contig: the consensus needs the complement table')
        arena = DeviceArena.adopt(self.lib.pw_graph_cons_arena_device(self.handle), self._count('pw_graph_cons_arena_bytes'), self.device,
                                  owner=self)
        return cstart, tasks, arena

    # ---- the later rounds of the consensus (include/pw_rounds.h) ----
    def consensus_relayout(self, polished, offsets, colmap, reads, complement=None, slack=50, drift=.1, stream=None):
        """``(cstart, tasks, arena)`` of the NEXT round (``pw_graph_consensus_relayout``; synchronous), like
        :meth:`consensus_layout`: ``polished`` are the polished contig letters one after another, ``offsets`` their
        ``n_unitigs + 1`` offsets and ``colmap`` the ``n_cols + 1`` entries of :meth:`biseqt_amd.batch.Pileup.colmap` over the
        current layout -- each a host array, or a device pointer (an ``int``, as the pileup's ``*_device`` accessors give
        it).  The placements are remapped through ``colmap`` and the tasks and the arena are laid out from the polished
        letters; :meth:`positions` and :meth:`lengths` then return the new round's values."""
        n_unitigs = self._count('pw_graph_num_unitigs')     # (raises before the first build)
        if not 0 <= int(slack) < 1 << 31:
            raise ValueError('slack must lie in 0 .. 2**31 - 1')
        if not (np.isfinite(drift) and 0 <= drift <= 1 << 20):
            raise ValueError('drift must be finite and lie in 0 .. 2**20')
        comp = None if complement is None else np.ascontiguousarray(complement, np.uint8).reshape(-1)
        if comp is not None and not 1 <= len(comp) <= 256:
            raise ValueError('complement must hold 1 .. 256 letters')
        held = []

        def dev(x, dtype):
            if isinstance(x, (int, np.integer)):
                return int(x)
            host = np.ascontiguousarray(x, dtype).reshape(-1)
            held.append(DeviceArena(host.view(np.uint8) if len(host) else np.zeros(8, np.uint8), self.device))
            return held[-1].ptr
        try:
            ptrs = dev(polished, np.uint8), dev(offsets, np.uint64), dev(colmap, np.uint64)
            src, offs, own = self._device_reads(reads)
            if own is not None:
                held.append(own)
            self._ck(self.lib.pw_graph_consensus_relayout(self.handle, ptrs[0], ptrs[1], ptrs[2], src.ptr, offs.ctypes.data,
                                                          None if comp is None else comp.ctypes.data, 0 if comp is None else len(comp),
                                                          int(slack), float(drift), stream), 'pw_graph_consensus_relayout')
        finally:
            for h in held:
                h.close()
        return self._layout_results(n_unitigs, comp)

    def round(self):
        """The round of the current layout: 1 after :meth:`consensus_layout`, one more per :meth:`consensus_relayout`."""
        n = int(self.lib.pw_graph_cons_round(self.handle))
        if n < 0:
            raise RuntimeError('pw_graph_cons_round failed: ' + W.last_error())
        return n

    def positions(self):
        """``int64[n_reads]``: where every read begins on its contig in the current round (0 for an unplaced read)."""
        return self._fetch('pw_graph_cons_positions', self.n_reads, np.int64)

    def lengths(self):
        """``int64[n_unitigs]``: the contig lengths of the current round."""
        return self._fetch('pw_graph_cons_lengths', self._count('pw_graph_num_unitigs'), np.int64)

    def _pile_tasks(self, pile, tasks, arena, alphabet_len, self_weight, max_cells, aligner_kw):
        """The self vote of the arena's columns and the alignments of ``tasks`` piled onto ``pile``, in batches of at most
        ``max_cells`` cells, the next batch planned while one runs.  Returns the number of tasks that aligned."""
        T, aligned = len(tasks), 0
        # frames: the windows, then the mutants
        offs = np.concatenate([tasks['col0'], tasks['mut_off']]).astype(np.int64)
        lens = np.concatenate([tasks['win_len'], self.read_lens[tasks['read']]]).astype(np.int64)
        pidx = np.stack([np.arange(T), T + np.arange(T)], 1).astype(np.int64)
        dr = np.stack([tasks['dmin'], tasks['dmax']], 1).astype(np.int64)
        cells = (dr[:, 1] - dr[:, 0] + 1) * np.minimum(lens[:T], lens[T:])
        csum, bounds, start = np.cumsum(cells), [], 0
        while start < T:
            base = csum[start - 1] if start else 0
            stop = max(start + 1, int(np.searchsorted(csum, base + max_cells, 'right')))
            bounds.append((start, stop)); start = stop
        kw = dict(match_score=1, mismatch_score=-3, go_score=-5, ge_score=-2)
        kw.update(aligner_kw)
        nothing = np.zeros(0, np.uint8)

        def create(lo, hi):
            return BatchAligner.from_arena(nothing, offs, lens, pidx[lo:hi], dr[lo:hi], device_arena=arena, alnmode=W.BANDED_MODE,
                                           alntype=W.B_OVERLAP, alphabet_len=alphabet_len, device=self.device,
                                           arena_bytes=arena.nbytes, **kw)

        pile.add_letters((arena, 0), weight=self_weight)
        cur = nxt = None
        try:
            nxt = create(*bounds[0]) if bounds else None
            for q, (lo, hi) in enumerate(bounds):
                cur, nxt = nxt, None
                cur.solve(); cur.traceback()               # asynchronous: the device is busy from here ...
                if q + 1 < len(bounds):
                    nxt = create(*bounds[q + 1])           # ... while the next batch is planned
                cur.pileup_add(pile, col0=tasks['col0'][lo:hi], sides='origin')
                cur.sync()
                aligned += int((cur.results()['opt_i'] >= 0).sum())
                cur.close(); cur = None
        finally:
            for b in (cur, nxt):
                if b is not None:
                    b.close()
        arena.read(0, 1)                                   # (a synchronous copy behind the last add)
        return aligned

    def consensus(self, reads, alphabet_len, complement=None, slack=50, drift=.1, min_depth=3, ins_slots=2, self_weight=1,
                  max_cells=2 * 10 ** 10, stats=None, rounds=1, **aligner_kw):
        """The polished contigs of the last build (include/pw_consensus.h): every read is placed on its contig, aligned
        (banded ``B_OVERLAP``, scores 1 / -3 / -5 / -2 unless ``aligner_kw`` says otherwise) against a window of the draft
        around its place -- ``slack + drift * len`` letters wider on either side, the band as wide around the nominal diagonal
        -- in batches of at most ``max_cells`` cells, the next batch planned while one runs; the alignments are piled onto the
        draft's columns, which vote for themselves with ``self_weight``, into a pileup with ``ins_slots`` insertion slots,
        and the pileup is polished with ``min_depth`` (the rule of include/pw_polish.h).  Only the tasks and the contig
        starts come to the host on the way: no draft letter and no transcript.  ``reads`` and ``complement`` as for
        :meth:`contigs`.  Returns ``(contigs, records)``: uint8 arrays in unitig order and one ``batch.POLISH_STATS_DTYPE``
        record per contig.  ``stats`` (a dict) receives ``placed``, ``unplaced``, ``tasks``, ``aligned`` and the times of the
        stages in ms, taken on the host around synchronised device work: ``layout_ms``, ``align_ms``, ``polish_ms``.

        ``rounds`` >= 2 (include/pw_rounds.h) iterates: the pileup is polished by columns, the placements are remapped
        through the coordinate map of that polish and the next round's tasks and arena are laid out from the polished letters
        where they are (:meth:`consensus_relayout`, from the pileup's device arrays), at most ``rounds`` times; a round whose
        records show no substitution, deletion or insertion on any contig has emitted its own input, and the loop stops
        there.  Between the rounds only offsets, records, tasks and contig starts come to the host.  The result is the last
        round's.  ``stats['rounds']`` lists, per round that ran, ``tasks``, ``aligned``, ``records``, ``layout_ms``,
        ``align_ms``, ``polish_ms``; ``tasks`` and ``aligned`` of ``stats`` itself are the last round's, the times are sums."""
        import time
        from .batch import POLISH_STATS_DTYPE, Pileup
        rounds = int(rounds)
        if rounds < 1:
            raise ValueError('rounds must be at least 1')
        t0 = time.perf_counter()
        cstart, tasks, arena = self.consensus_layout(reads, complement=complement, slack=slack, drift=drift)
        lengths = self.unitigs()[0]['length'].astype(np.int64)
        t1 = time.perf_counter()
        per_round = []
        for k in range(1, rounds + 1):
            n_cols, T = int(cstart[-1]), len(tasks)
            aligned, nxt = 0, None
            if n_cols == 0:
                out, offsets, records = np.zeros(0, np.uint8), np.zeros(len(lengths) + 1, np.int64), np.zeros(len(lengths), POLISH_STATS_DTYPE)
                t2 = t3 = t4 = t1
                last = True
            else:
                with Pileup(n_cols, alphabet_len, device=self.device, ins_slots=ins_slots) as pile:
                    aligned = self._pile_tasks(pile, tasks, arena, alphabet_len, self_weight, max_cells, aligner_kw)
                    t2 = time.perf_counter()
                    if rounds == 1:
                        out, offsets, records = pile.polish((arena, 0), cstart[:-1], lengths, min_depth=min_depth)
                    else:
                        offsets, records = pile._polish((arena, 0), cstart[:-1], lengths, min_depth, None, True, False)
                    t3 = t4 = time.perf_counter()
                    last = k == rounds or not (records['substituted'].any() or records['deleted'].any() or records['inserted'].any())
                    if last and rounds > 1:
                        out = pile.polished_letters()
                    elif not last:                             # (before the pileup closes: its arrays are the relayout's input)
                        nxt = self.consensus_relayout(int(self.lib.pw_pileup_polished_letters_device(pile.handle)),
                                                      int(self.lib.pw_pileup_polished_offsets_device(pile.handle)),
                                                      int(self.lib.pw_pileup_colmap_device(pile.handle)), reads, complement=complement,
                                                      slack=slack, drift=drift)
                        t4 = time.perf_counter()
            per_round.append(dict(tasks=T, aligned=aligned, records=records, layout_ms=1e3 * (t1 - t0), align_ms=1e3 * (t2 - t1),
                                  polish_ms=1e3 * (t3 - t2)))
            if last:
                break
            (cstart, tasks, arena), lengths = nxt, np.diff(offsets).astype(np.int64)
            t0, t1 = t3, t4
        if stats is not None:
            place = self._fetch('pw_graph_placements', self.n_reads, PLACE_DTYPE)
            stats.update(placed=int((place['unitig'] >= 0).sum()), unplaced=int((place['unitig'] < 0).sum()), tasks=per_round[-1]['tasks'],
                         aligned=per_round[-1]['aligned'], rounds=per_round,
                         **{key: sum(r[key] for r in per_round) for key in ('layout_ms', 'align_ms', 'polish_ms')})
        return [out[offsets[u]:offsets[u + 1]].copy() for u in range(len(lengths))], records
