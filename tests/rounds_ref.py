"""CPU oracle of the iterated consensus (include/pw_rounds.h restated in plain Python): the polish one column at a time with
the draft->polished coordinate map it yields, the remap of the placements through that map, the next round's layout, and the
whole flow of rounds on the oracle side.  Built from tests/polish_ref.py (the rule, a column at a time) and
tests/consensus_ref.py (tasks and arena, which take placements and ``(.., length, ..)`` unitig tuples as plain data)."""
import numpy as np

from tests import consensus_cases as CC
from tests import consensus_ref as CR
from tests import graph_ref as GR
from tests import polish_cases as PC
from tests import polish_ref as PR


def column_polish(counts, ins, L, letters, offs, lens, min_depth=1):
    """``(reads, stats, colmap)``: what ``polish_ref.polish`` gives, computed column by column, and ``colmap`` (uint64,
    ``n_cols + 1``): the exclusive sums of the letters every column emits, 0 for a column that lies in no read.  The reads
    must come in column order and must not overlap."""
    n_cols = len(counts)
    offs, lens = [int(x) for x in offs], [int(x) for x in lens]
    for r, (off, n) in enumerate(zip(offs, lens)):
        if n < 0 or off < 0 or off + n > n_cols:
            raise ValueError('read %d lies outside the pileup' % r)
        if r + 1 < len(offs) and off + n > offs[r + 1]:
            raise ValueError('read %d overlaps read %d or comes behind it' % (r, r + 1))
    e = np.zeros(n_cols + 1, np.uint64)
    reads, stats = [], np.zeros(len(offs), PR.STATS_DTYPE)
    for r, (off, n) in enumerate(zip(offs, lens)):
        out, rec = [], np.zeros(4, np.int64)
        for c in range(off, off + n):
            (col,), st = PR.polish(counts, ins, L, letters, [c], [1], min_depth)
            e[c] = len(col)
            out.extend(col)
            rec += np.array(st[0].tolist(), np.int64)
        reads.append(out)
        stats[r] = tuple(rec.tolist())
    colmap = np.zeros(n_cols + 1, np.uint64)
    colmap[1:] = np.cumsum(e[:-1], dtype=np.uint64)
    return reads, stats, colmap


def remap(pos, n, emap):
    """ROUND REMAP for one position on a contig of ``n`` letters; ``emap`` has ``n + 1`` entries, ``emap[0] == 0``."""
    pos, n = int(pos), int(n)
    if pos < 0:
        return pos
    if pos <= n:
        return int(emap[pos])
    return int(emap[n]) + (pos - n)


def next_round(lens, places, lengths, cstart, colmap, polished, reads, slack, drift, complement=None):
    """RELAYOUT: ``polished`` are the polished contigs (in unitig order) of a column polish over the layout
    ``(lengths, cstart)`` that gave ``colmap``.  Returns ``dict(places, lengths, tasks, cstart, arena_bytes, arena)`` of the
    next round."""
    colmap = [int(x) for x in colmap]
    emaps = [[colmap[cstart[u] + x] - colmap[cstart[u]] for x in range(int(n) + 1)] for u, n in enumerate(lengths)]
    new_len = [em[-1] for em in emaps]
    assert new_len == [len(c) for c in polished], (new_len, [len(c) for c in polished])
    new_places = []
    for (u, rev, pos, root, depth) in places:
        new_places.append((u, rev, pos, root, depth) if u < 0 else (u, rev, remap(pos, lengths[u], emaps[u]), root, depth))
    unitigs = [(0, n, 0, 0, 0) for n in new_len]
    task_list, cs, arena_bytes = CR.tasks(lens, new_places, unitigs, slack, drift)
    arena = CR.arena(reads, polished, task_list, cs, arena_bytes, complement)
    return dict(places=new_places, lengths=new_len, tasks=task_list, cstart=cs, arena_bytes=arena_bytes, arena=arena)


def _one_round(oracle, lens, lay, min_depth, ins_slots, self_weight):
    """Align, pile and column-polish one layout ``dict(lengths, tasks, cstart, arena)``."""
    cstart, arena, task_list = lay['cstart'], lay['arena'], lay['tasks']
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
    polished, stats, colmap = column_polish(counts, ins, PC.L, arena, cstart[:-1], lay['lengths'], min_depth)
    return dict(contigs=[np.array(c, np.uint8) for c in polished], stats=stats, colmap=colmap, aligned=aligned, tasks=task_list,
                cstart=cstart, lengths=list(lay['lengths']), places=lay['places'])


def oracle_rounds(oracle, reads, records, rounds, slack=CC.SLACK, drift=CC.DRIFT, min_depth=PC.MIN_DEPTH, ins_slots=PC.INS_SLOTS,
                  self_weight=PC.SELF_WEIGHT, graph_params=None):
    """The whole flow on the oracle side: at most ``rounds`` rounds of align, pile, column polish and relayout, stopping behind
    the first round whose records show no substitution, deletion or insertion on any contig.  Returns ``(draft, rounds)``:
    the draft contigs and one dict per round that ran (contigs, stats, colmap, aligned, tasks, cstart, lengths, places)."""
    lens = [len(r) for r in reads]
    built = GR.build(lens, records, **(graph_params or {}))
    draft = [np.array(c, np.uint8) for c in GR.contigs(reads, built['unitigs'], built['members'], CC.COMPLEMENT)]
    places = CR.place(lens, records, built)
    task_list, cstart, arena_bytes = CR.tasks(lens, places, built['unitigs'], slack, drift)
    lay = dict(places=places, lengths=[u[1] for u in built['unitigs']], tasks=task_list, cstart=cstart,
               arena=CR.arena(reads, draft, task_list, cstart, arena_bytes, CC.COMPLEMENT))
    out = []
    for k in range(rounds):
        got = _one_round(oracle, lens, lay, min_depth, ins_slots, self_weight)
        out.append(got)
        st = got['stats']
        if k + 1 == rounds or not (st['substituted'].any() or st['deleted'].any() or st['inserted'].any()):
            break
        lay = next_round(lens, lay['places'], lay['lengths'], lay['cstart'], got['colmap'], got['contigs'], reads, slack, drift,
                         CC.COMPLEMENT)
    return draft, out
