"""Seeds -> segments -> banded DP extension, everything heavy on the GPU.

The reference has no library function for this; the flow is written out in its experiments
(``experiments/blot_stats.py:374-470``): Word-Blot finds the similar segments of a pair of sequences, every segment
is turned into a pair of sub-frames a few word lengths larger, and a banded global alignment of the two frames is
solved, traced back and truncated to its first / last match.  Here the frames of ALL segments are solved by one
batch (`BatchAligner`), i.e. a handful of kernel launches, and the arithmetic that decides the frames and bands is
the reference's, statement by statement.  ``map_queries`` is the many-queries-one-reference flow of
``experiments/blot_ig_genotyping.py``: segments of all queries from one pass, one banded local batch.
"""
import numpy as np

from . import _pwlib as W
from .batch import BatchAligner, DeviceArena, Pileup, cigar_strings, pack_reads, summary_dict
from .blot import WordBlot, WordBlotLocalRef
from .overlap import _complement
from .pw import Alignment
from .sequence import Sequence, reverse_complement


def segment_frame(seg, lenS, lenT, wordlen):
    """Frames ``(i_start, i_end), (j_start, j_end)`` and band radius for one similar segment
    ``((d_min, d_max), (a_min, a_max))`` -- ``experiments/blot_stats.py:438-453``."""
    (i_start, i_end), (j_start, j_end) = WordBlot.to_ij_coordinates_seg(seg)
    i_end = min(lenS - 1, i_end)                       # to_ij_coordinates_seg might overflow
    j_end = min(lenT - 1, j_end)
    start_shift = min(i_start, j_start, 2 * wordlen)   # allow longer alignments to be found
    end_shift = min(lenS - i_end, lenT - j_end, 2 * wordlen)
    i_start, j_start = i_start - start_shift, j_start - start_shift
    i_end, j_end = i_end + end_shift, j_end + end_shift
    n_s, n_t = i_end - i_start, j_end - j_start
    rad = (seg[0][1] - seg[0][0]) // 2
    rad = min(n_s, n_t, max(rad, abs(n_s - n_t) + 2))
    return (i_start, i_end), (j_start, j_end), rad


def truncated_frame(origin_start, mutant_start, summary):
    """``((origin_start, origin_end), (mutant_start, mutant_end))`` of the sub-alignment between the first and the last
    ``M`` of a transcript, from its summary record and the alignment's starts -- the starts of
    ``Alignment.truncate_to_match()`` and the letters its transcript consumes -- or None where ``truncate_to_match`` returns
    None (at most one ``M``) or fails (no ``M``, no transcript)."""
    if not summary['flags'] & 1 or summary['first_match'] < 0 or summary['first_match'] >= summary['last_match']:
        return None
    o0, m0 = origin_start + summary['head_origin'], mutant_start + summary['head_mutant']
    on_origin = summary['n_match'] + summary['n_subst'] + summary['n_del'] - summary['head_origin'] - summary['tail_origin']
    on_mutant = summary['n_match'] + summary['n_subst'] + summary['n_ins'] - summary['head_mutant'] - summary['tail_mutant']
    return (o0, o0 + on_origin), (m0, m0 + on_mutant)


def extend_segments(S, T, segments, wordlen, device=0, alignments=True, **aligner_kw):
    """Banded alignment of the frames of all ``segments`` (dicts with a ``segment`` key, as
    ``WordBlot.similar_segments`` yields them) in one GPU batch.  ``aligner_kw`` are ``Aligner`` keywords
    (``alnmode`` / ``alntype`` default to banded global as in the reference's experiment; ``diag_range`` is set
    per segment).  Returns one dict per segment: ``frame``, ``diag_range``, ``score``, ``alignment`` (an
    :class:`Alignment` on the frame sequences, or None), ``truncated`` (``alignment.truncate_to_match()``) and ``kernel``
    (the batch's fill kernel and score type, for diagnostics).

    With ``alignments=False`` no transcript leaves the device: ``alignment`` and ``truncated`` are None and every dict has
    ``summary`` (the fields of ``batch.SUMMARY_DTYPE``, None without an alignment) and ``truncated_frame``, the frame
    coordinates ``((origin_start, origin_end), (mutant_start, mutant_end))`` of what ``truncated`` would cover
    (:func:`truncated_frame`), both from the summaries the device reduces from the ops."""
    assert isinstance(S, Sequence) and isinstance(T, Sequence)
    kw = dict(alnmode=W.BANDED_MODE, alntype=W.B_GLOBAL)
    kw.update(aligner_kw)
    assert kw['alnmode'] == W.BANDED_MODE, 'segments are extended by banded alignments'
    s, t = S.as_array(np.uint8), T.as_array(np.uint8)
    frames, pairs, bands = [], [], []
    for rec in segments:
        fi, fj, rad = segment_frame(rec['segment'], len(S), len(T), wordlen)
        frames.append((fi, fj))
        pairs.append((s[fi[0]:fi[1]], t[fj[0]:fj[1]]))
        bands.append((-rad, rad))
    if not frames:
        return []
    kw.pop('diag_range', None)
    with BatchAligner(pairs, alphabet_len=len(S.alphabet), diag_range=bands, device=device, **kw) as b:
        if alignments:
            res = b.run()
            txs = b.transcripts(res)
        else:
            res, sums = _run_summarized(b)
        kernel = (b.kernel_name, b.score_dtype)
    out = []
    for k, (fi, fj) in enumerate(frames):
        rec = {'frame': (fi, fj), 'diag_range': bands[k], 'score': None, 'alignment': None, 'truncated': None, 'kernel': kernel}
        if not alignments:
            rec['summary'] = rec['truncated_frame'] = None
            if res['opt_i'][k] >= 0 and res['tx_len'][k] > 0:
                rec['score'] = float(res['score'][k])
                rec['summary'] = summary_dict(sums[k])
                rec['truncated_frame'] = truncated_frame(int(res['origin_idx'][k]), int(res['mutant_idx'][k]), rec['summary'])
        elif res['opt_i'][k] >= 0 and txs[k]:
            rec['score'] = float(res['score'][k])
            aln = Alignment(S[fi[0]:fi[1]], T[fj[0]:fj[1]], txs[k], score=rec['score'],
                            origin_start=int(res['origin_idx'][k]), mutant_start=int(res['mutant_idx'][k]))
            rec['alignment'] = aln
            rec['truncated'] = aln.truncate_to_match() if 'M' in txs[k] else None
        out.append(rec)
    return out


def _run_summarized(b):
    """solve -> traceback -> summarize on one batch: the 32-byte records and the 48-byte summaries, no transcript."""
    b.solve()
    b.traceback()
    b.summarize()
    b.sync()
    res = b.results()
    return res, b.summaries()


def rank_segments(segments, keep):
    """The best ``keep`` of one query's segments (dicts with ``p`` and ``segment``) by ``p * (a_max - a_min)``, best first
    (``experiments/blot_ig_genotyping.py:45-48, 72-75``).  The sort is stable: with the plus strand's segments listed before
    the minus strand's, as ``similar_segments_many(strands='both')`` lists them, a tie goes to ``'+'``."""
    return sorted(segments, key=lambda rec: -(rec['p'] * (rec['segment'][1][1] - rec['segment'][1][0])))[:keep]


def query_interval(strand, mutant_start, len_aln, query_len):
    """The half-open interval of the query AS GIVEN that an alignment covers: it starts at ``mutant_start`` of the aligned
    sequence and consumes ``len_aln`` of its letters.  On ``'+'`` the aligned sequence is the query; on ``'-'`` it is
    ``rc(query)`` and the interval is the one :func:`biseqt_amd.overlap.minus_to_forward` returns for the transcript, here
    from the number of letters alone (the op counts stand in where no transcript comes to the host)."""
    assert strand in ('+', '-') and 0 <= mutant_start and len_aln >= 0 and mutant_start + len_aln <= query_len
    if strand == '+':
        return mutant_start, mutant_start + len_aln
    return query_len - (mutant_start + len_aln), query_len - mutant_start


def pileup_col0(res, per_query, which):
    """The ``col0`` array of :meth:`BatchAligner.pileup_add` for the batch of :func:`map_queries`: 0 for a chosen record, -1
    for the others.  ``res`` are the batch's records (query by query, rank order within a query), ``per_query`` the number
    of records of every query.  A record has an alignment when ``opt_i >= 0 and tx_len > 0``.  ``which`` = ``'all'`` chooses
    every such record, ``'best'`` per query the one with the highest score, a tie going to the earlier one."""
    has = (np.asarray(res['opt_i']) >= 0) & (np.asarray(res['tx_len']) > 0)
    col0 = np.full(len(has), -1, np.int64)
    if which == 'all':
        col0[has] = 0
        return col0
    k = 0
    for n in per_query:
        best = None
        for r in range(k, k + n):
            if has[r] and (best is None or res['score'][r] > res['score'][best]):
                best = r
        if best is not None:
            col0[best] = 0
        k += n
    return col0


def map_queries(ref, queries, K_min, p_min, wordlen, g_max, sensitivity, keep=3, device=0, aligner_kw=None, alignments=True,
                strands='+', complement=None, cigar=None, pileup=None, pileup_records='best'):
    """Map many short queries onto one reference sequence: Word-Blot local similarities of all queries in one pass
    (:meth:`WordBlotLocalRef.similar_segments_many`), then a banded local alignment of the best segments of every query,
    all in ONE lane-packed batch.  The flow of ``experiments/blot_ig_genotyping.py:45-101`` as a library function: per
    query the segments are ranked by ``p * (a_max - a_min)`` (:45-48), the best ``keep`` are kept (:72-75) and aligned
    inside ``diag_range = (int(d_min), int(d_max))`` of the segment (:79-88).  Default scores are 1 / -3 / -5 / -2
    (match, mismatch, gap open, gap extend).

    Returns one list per query, best segment first, of dicts: ``segment``, ``p``, ``diag_range``, ``score``,
    ``alignment`` (an :class:`Alignment` on ``ref`` and the query, or None where the batch reports no alignment),
    ``p_aln`` (matches over the letters of the query the alignment covers, rounded to 2 places) and ``len_aln`` (:93-98).

    With ``alignments=False`` only the 32-byte records and the 48-byte summaries of the batch come to the host -- no
    transcript is downloaded or decoded: ``alignment`` is None, ``p_aln`` and ``len_aln`` come from the op counts, and every
    dict also has ``origin_start``, ``mutant_start`` (those of the :class:`Alignment`) and ``summary`` (the fields of
    ``batch.SUMMARY_DTYPE``; None where there is no alignment).

    ``strands``: ``'+'`` (the default, with exactly the keys above), ``'-'`` or ``'both'``; ``complement`` as in
    :meth:`WordBlotLocalRef.similar_segments_many`.  A record on the minus strand maps ``T = rc(query)`` -- position ``j'``
    of ``T`` is letter ``len - 1 - j'`` of the query, complemented; the convention :mod:`biseqt_amd.overlap` documents --
    and its segment, ``diag_range``, start indices and transcript are in the frame of that ``T``: they equal what the
    default call returns for the materialised ``rc(query)``, and ``alignment`` is
    ``Alignment(ref, reverse_complement(query), ...)``.  A query's segments of the selected strands are ranked together
    (:func:`rank_segments`: a tie goes to ``'+'``) and the best ``keep`` aligned in the one batch.  Every record then also
    has ``strand`` and ``query_interval``: the half-open interval of the query AS GIVEN that the alignment covers
    (:func:`query_interval`; None without an alignment).  The seeding reads the forward letters only; for the alignment
    step the device writes the reverse complement of every query behind the uploaded letters, once, before the seeding.

    ``cigar``: None (the default: exactly the keys above and no further launch), ``'extended'`` (``=`` / ``X``) or
    ``'classic'`` (``M``).  Every record then also has ``cigar``: the alignment as a CIGAR string with ``ref`` as the target
    and the aligned sequence as the query (None without an alignment), run-length encoded on the device from the ops
    (:meth:`BatchAligner.cigars`) in both ``alignments=`` modes -- with ``alignments=False`` still no transcript leaves the
    device.  On the minus strand the CIGAR is in the frame of ``T = rc(query)`` against the forward reference, which is PAF's
    and SAM's convention for ``-``: nothing is reversed.

    ``pileup``: None (the default: no further launch, identical output) or a :class:`biseqt_amd.batch.Pileup` with
    ``n_cols == len(ref)`` and the reference's alphabet length, on ``device``.  Behind the batch's traceback the records
    ``pileup_records`` names add their ops to the columns of ``ref`` (:meth:`BatchAligner.pileup_add`; column = reference
    position) without a transcript leaving the device: ``'best'`` -- per query the record with an alignment and the highest
    score, a tie going to the earlier one in rank order -- or ``'all'`` -- every record with an alignment.  It works in both
    ``alignments=`` modes, with any ``strands`` and any ``cigar``; a minus-strand record piles the letters of ``rc(query)``
    onto the forward reference, which is what its frame already is.  The function returns what it returns without
    ``pileup``; the caller owns the pileup (adding is cumulative: several calls may add to one) and reads it with
    ``counts()``, or ``call()`` and ``sites()`` / ``consensus()`` / ``variants()``."""
    assert isinstance(ref, Sequence) and all(isinstance(T, Sequence) for T in queries)
    queries = list(queries)
    if strands not in ('+', '-', 'both'):
        raise ValueError("strands is '+', '-' or 'both', not %r" % (strands,))
    if cigar not in (None, 'extended', 'classic'):
        raise ValueError("cigar is None, 'extended' or 'classic', not %r" % (cigar,))
    if pileup_records not in ('best', 'all'):
        raise ValueError("pileup_records is 'best' or 'all', not %r" % (pileup_records,))
    if pileup is not None:
        if not isinstance(pileup, Pileup) or not pileup.handle:
            raise ValueError('pileup must be an open biseqt_amd.batch.Pileup')
        if pileup.n_cols != len(ref) or pileup.alphabet_len != len(ref.alphabet) or pileup.device != device:
            raise ValueError('pileup must have n_cols == len(ref) = %d and alphabet_len %d, on device %d'
                             % (len(ref), len(ref.alphabet), device))
    stranded = strands != '+'
    kw = dict(match_score=1, mismatch_score=-3, go_score=-5, ge_score=-2)
    kw.update(aligner_kw or {})
    kw.pop('diag_range', None)
    kw.update(alnmode=W.BANDED_MODE, alntype=W.B_LOCAL)
    arena, offs, lens = pack_reads([ref] + queries)           # read 0 is the reference, read 1 + q is query q
    nq = len(queries)
    if stranded:                                              # ... and frame 1 + nq + q is rc(query q), written by the device
        comp = _complement(complement, len(ref.alphabet), ref.alphabet)
        darena = DeviceArena.with_reverse_complements(arena, offs, lens, np.arange(1, 1 + nq), comp, device)
        all_offs, all_lens = np.concatenate([offs, darena.rc_offsets]), np.concatenate([lens, lens[1:]])
        seed_kw = dict(strands=strands, complement=comp)
    else:
        darena, all_offs, all_lens, seed_kw = DeviceArena(arena, device=device), offs, lens, {}
    out = [[] for _ in queries]
    with darena:
        wb = WordBlotLocalRef(ref, alphabet=ref.alphabet, wordlen=wordlen, g_max=g_max, sensitivity=sensitivity, device=device)
        try:
            segs = wb.similar_segments_many(queries, K_min, p_min, arena=(darena, offs[1:], lens[1:]), **seed_kw)
        finally:
            wb.close()
        pairs, bands = [], []
        for q, recs in enumerate(segs):
            for seg in rank_segments(recs, keep):
                d_band = seg['segment'][0]
                rec = dict(segment=seg['segment'], p=seg['p'], diag_range=(int(d_band[0]), int(d_band[1])), score=None,
                           alignment=None, p_aln=None, len_aln=None)
                if not alignments:
                    rec.update(origin_start=None, mutant_start=None, summary=None)
                if stranded:
                    rec.update(strand=seg['strand'], query_interval=None)
                if cigar is not None:
                    rec.update(cigar=None)
                out[q].append(rec)
                pairs.append((0, 1 + q + (nq if stranded and seg['strand'] == '-' else 0)))
                bands.append(rec['diag_range'])
        if not pairs:
            return out
        with BatchAligner.from_arena(arena, all_offs, all_lens, pairs, diag_ranges=bands, device_arena=darena,
                                     alphabet_len=len(ref.alphabet), device=device, arena_bytes=darena.nbytes, **kw) as b:
            if alignments:
                res = b.run()
                txs = b.transcripts(res)
            else:
                res, sums = _run_summarized(b)
            if cigar is not None:
                cgs = cigar_strings(*b.cigars(cigar))
            if pileup is not None:
                # the reference is read 0 at arena offset 0: a chosen record's frame starts at column 0
                b.pileup_add(pileup, col0=pileup_col0(res, [len(recs) for recs in out], pileup_records))
                b.sync()
    k = 0
    for q, recs in enumerate(out):
        for rec in recs:
            mutant_start = int(res['mutant_idx'][k])
            if not alignments:
                if res['opt_i'][k] >= 0 and res['tx_len'][k] > 0:
                    s = sums[k]
                    rec['score'] = float(res['score'][k])
                    rec['origin_start'], rec['mutant_start'] = int(res['origin_idx'][k]), mutant_start
                    len_on_query = int(s['n_match']) + int(s['n_subst']) + int(s['n_ins'])
                    rec['p_aln'] = round(1. * int(s['n_match']) / len_on_query, 2) if len_on_query else None
                    rec['len_aln'] = len_on_query
                    rec['summary'] = summary_dict(s)
            elif res['opt_i'][k] >= 0 and txs[k]:
                tx = txs[k]
                rec['score'] = float(res['score'][k])
                T = reverse_complement(queries[q], comp) if stranded and rec['strand'] == '-' else queries[q]
                rec['alignment'] = Alignment(ref, T, tx, score=rec['score'], origin_start=int(res['origin_idx'][k]),
                                             mutant_start=mutant_start)
                len_on_query = sum(tx.count(op) for op in 'MSI')
                rec['p_aln'] = round(1. * tx.count('M') / len_on_query, 2) if len_on_query else None
                rec['len_aln'] = len_on_query
            if cigar is not None and rec['score'] is not None:
                rec['cigar'] = cgs[k] or None
            if stranded and rec['len_aln'] is not None:
                rec['query_interval'] = query_interval(rec['strand'], mutant_start, rec['len_aln'], len(queries[q]))
            k += 1
    return out


def paf_lines(mapped, ref_name, ref_len, query_names, query_lens):
    """The records of :func:`map_queries` (either ``alignments=`` mode, any ``strands``) as PAF: one line -- a ``str`` without
    the newline -- per record that has an alignment, in the order of ``mapped``.  ``ref`` is the target.  Columns: query name,
    query length, query start and end on the query AS GIVEN (``query_interval``; without strands ``mutant_start`` and
    ``mutant_start + len_aln``), strand (``+`` for a record without a ``strand`` key), target name, target length, target start
    (``origin_start``), target end (start + the letters of ``ref`` the alignment consumes), matches, alignment length (every
    op), mapping quality 255 (not available).  Tags: ``AS:i:`` for an integral score, ``AS:f:`` for any other, and ``cg:Z:``
    when the record has ``cigar``.  The op counts come from ``summary`` where there is one, otherwise from the transcript."""
    lines = []
    for q, recs in enumerate(mapped):
        for rec in recs:
            if rec['score'] is None:
                continue
            aln = rec.get('alignment')
            if rec.get('summary') is not None:
                n_match, n_subst, n_ins, n_del = (int(rec['summary'][f]) for f in ('n_match', 'n_subst', 'n_ins', 'n_del'))
            else:
                n_match, n_subst, n_ins, n_del = (aln.transcript.count(op) for op in 'MSID')
            origin_start = rec['origin_start'] if aln is None else aln.origin_start
            mutant_start = rec['mutant_start'] if aln is None else aln.mutant_start
            if 'strand' in rec:
                strand, (q_start, q_end) = rec['strand'], rec['query_interval']
            else:
                strand, q_start, q_end = '+', mutant_start, mutant_start + rec['len_aln']
            score = float(rec['score'])
            cols = [query_names[q], int(query_lens[q]), q_start, q_end, strand, ref_name, int(ref_len), origin_start,
                    origin_start + n_match + n_subst + n_del, n_match, n_match + n_subst + n_ins + n_del, 255,
                    'AS:i:%d' % int(score) if score == int(score) else 'AS:f:%r' % score]
            if rec.get('cigar'):
                cols.append('cg:Z:' + rec['cigar'])
            lines.append('\t'.join(str(c) for c in cols))
    return lines


def local_homology_scan(S, T, K_min, p_min, wordlen, g_max=.3, sensitivity=.99, mask=(), device=0,
                        aligner_kw=None):
    """Word-Blot local-homology scan followed by banded DP extension of every similar segment (BASELINE config 5;
    ``experiments/blot_stats.py:362-470``).  Default scores are the experiment's: match ``1 / p_min - 1``,
    mismatch -1, gap extend -1, gap open 0, banded global.  Returns ``(segments, extensions)``."""
    if aligner_kw is None:
        aligner_kw = dict(match_score=1. / p_min - 1, mismatch_score=-1, ge_score=-1, go_score=0)
    wb = WordBlot(S, T, g_max=g_max, sensitivity=sensitivity, alphabet=S.alphabet, wordlen=wordlen, mask=list(mask),
                  device=device)
    try:
        segments = list(wb.similar_segments(K_min, p_min))
    finally:
        wb.close()
    return segments, extend_segments(S, T, segments, wordlen, device=device, **aligner_kw)
