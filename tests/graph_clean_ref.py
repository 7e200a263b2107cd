"""CPU oracle of the graph cleaning: the CLEANING paragraph of include/pw_graph.h and the ``Dropped reads`` paragraph of
include/pw_consensus.h restated in plain Python, with dict look-ups and explicit components -- no doubling, no per-head
tables.  Classification, arcs, the row index and the reduction are those of tests/graph_ref.py; what is new here is the
decomposition over the LIVE vertices, the two rules, the rounds, the final unitig pass and the parents of dropped reads.
Records and results have the shapes of tests/graph_ref.py and tests/consensus_ref.py; ``build`` adds ``dropped``."""
from tests import consensus_ref as CR
from tests import graph_ref as R

REDUCED, REMOVED, CHAIN, DROPPED = R.REDUCED, R.REMOVED, R.CHAIN, 8
TIP, BUBBLE = 1, 2


def _decompose(arcs, V, live):
    """UNITIGS over the live vertices: ``(out, leaving, entering, succ, adv, links, comps)``; ``leaving[v]`` / ``entering[v]``
    list the other end of every kept arc (one entry per arc), ``links`` the arc indices of the chain links, ``comps`` the
    ``(path, circular)`` pairs, a cycle rotated to its smallest vertex."""
    out = [0] * V
    leaving, entering = {}, {}
    for v, w, _, _, _, f in arcs:
        if not f & REMOVED:
            out[v] += 1
            leaving.setdefault(v, []).append(w)
            entering.setdefault(w, []).append(v)
    for v in range(V):                                       # in(v) = out(v ^ 1): REMOVED is twin-symmetric
        assert len(entering.get(v, [])) == out[v ^ 1]
    succ, pred, adv, links = {}, {}, {}, []
    for s, (v, w, ln, _, _, f) in enumerate(arcs):
        if not f & REMOVED and out[v] == 1 and out[w ^ 1] == 1 and w != v and w != v ^ 1:
            assert v not in succ and w not in pred
            succ[v], pred[w], adv[v] = w, v, ln
            links.append(s)
    seen, comps = set(), []
    for v in range(V):
        if not live[v >> 1] or v in seen:
            continue
        head = v
        while head in pred and pred[head] != v:
            head = pred[head]
        circular = head in pred
        path = [head]
        while path[-1] in succ and succ[path[-1]] != head:
            path.append(succ[path[-1]])
        if circular:
            k = path.index(min(path))
            path = path[k:] + path[:k]
        assert all(live[x >> 1] for x in path)
        seen.update(path)
        comps.append((path, circular))
    return out, leaving, entering, succ, adv, links, comps


def _round(arcs, V, live, dropped, max_tip_reads, max_bubble_reads):
    out, leaving, entering, _, _, _, comps = _decompose(arcs, V, live)
    comp_of = {v: k for k, (path, _) in enumerate(comps) for v in path}
    n = [len(path) for path, _ in comps]
    mr = [min(path) >> 1 for path, _ in comps]
    head = [path[0] for path, _ in comps]
    tail = [path[-1] for path, _ in comps]
    twin = [comp_of[path[-1] ^ 1] for path, _ in comps]
    for k, (path, circular) in enumerate(comps):
        if not circular:
            assert comps[twin[k]][0] == [v ^ 1 for v in reversed(path)]
        assert n[twin[k]] == n[k] and mr[twin[k]] == mr[k]

    def in_(v):
        return out[v ^ 1]

    tip = [max_tip_reads > 0 and not circ and n[k] <= max_tip_reads and in_(head[k]) == 0 and out[tail[k]] >= 1
           for k, (_, circ) in enumerate(comps)]
    ends = {}
    for k, (_, circ) in enumerate(comps):
        h, t = head[k], tail[k]
        if max_bubble_reads > 0 and not circ and n[k] <= max_bubble_reads and in_(h) == 1 and out[t] == 1:
            s, z = entering[h][0], leaving[t][0]
            if not {s >> 1, z >> 1} & {h >> 1, t >> 1}:
                ends[k] = (s, z)
    verdict = {}
    for k in range(len(comps)):
        if tip[k]:
            t = tail[k]
            for w in leaving[t]:
                for u in entering[w]:
                    if u == t:
                        continue
                    d = comp_of[u]
                    assert tail[d] == u and not comps[d][1]      # the competitor is the tail of a linear component
                    if not tip[d] or n[d] > n[k] or (n[d] == n[k] and mr[d] < mr[k]):
                        verdict[k] = TIP
        if k in ends:
            for d in ends:
                if d != k and ends[d] == ends[k] and (n[d] > n[k] or (n[d] == n[k] and mr[d] < mr[k])):
                    verdict[k] = BUBBLE
    # the decisions for C and C ^ 1 never contradict each other
    for k in range(len(comps)):
        assert not (tip[k] and k in ends)
        assert not (tip[k] and tip[twin[k]]) or twin[k] == k
        assert (k in ends) == (twin[k] in ends)
        assert (verdict.get(k) == BUBBLE) == (verdict.get(twin[k]) == BUBBLE)
        assert not (verdict.get(k) == TIP and verdict.get(twin[k]) == BUBBLE)
    for k, kind in verdict.items():
        for v in comps[k][0]:
            assert dropped[v >> 1] in (0, kind)
            dropped[v >> 1] = kind
            live[v >> 1] = False
    for arc in arcs:
        if not arc[5] & REMOVED and (dropped[arc[0] >> 1] or dropped[arc[1] >> 1]):
            arc[5] |= REMOVED | DROPPED


def build(lens, records, max_hang=1000, int_frac=.8, min_overlap=0, min_identity=0., fuzz=10, max_tip_reads=0, max_bubble_reads=0,
          rounds=1):
    """``graph_ref.build``'s dict plus ``dropped`` (one per read: 0, 1 tip, 2 bubble)."""
    if max_tip_reads < 0 or max_bubble_reads < 0 or not 0 <= rounds <= 8:
        raise ValueError('max_tip_reads and max_bubble_reads must not be negative, rounds must lie in 0 .. 8')
    lens = [int(x) for x in lens]
    base = R.build(lens, records, max_hang=max_hang, int_frac=int_frac, min_overlap=min_overlap, min_identity=min_identity, fuzz=fuzz)
    V = 2 * len(lens)
    arcs = [list(a[:5]) + [a[5] & ~CHAIN] for a in base['arcs']]
    live = [not c for c in base['contained']]
    dropped = [0] * len(lens)
    for _ in range(rounds if (max_tip_reads > 0 or max_bubble_reads > 0) else 0):
        _round(arcs, V, live, dropped, max_tip_reads, max_bubble_reads)
    assert all(live[r] == (not base['contained'][r] and not dropped[r]) for r in range(len(lens)))
    _, _, _, _, adv, links, comps = _decompose(arcs, V, live)
    for s in links:
        arcs[s][5] |= CHAIN
    unitigs, members = [], []
    for path, circular in sorted((c for c in comps if min(c[0]) % 2 == 0), key=lambda c: c[0][0]):
        first, off = len(members), 0
        for k, v in enumerate(path):
            step = adv[v] if (k + 1 < len(path) or circular) else lens[v >> 1]
            members.append((v, step, off))
            off += step
        unitigs.append((first, off, len(path), path[0], int(circular)))
    return dict(cls=base['cls'], contained=base['contained'], dropped=dropped, arcs=[tuple(a) for a in arcs], rows=base['rows'],
                unitigs=unitigs, members=members)


def parent_links(lens, records, built):
    """``consensus_ref.parent_links`` plus the parent of every dropped read: the dovetail record with the largest n_match (a tie
    to the lowest index) that joins it to a live read; the dropped read is the child, rows "child a" / "child b" of the table."""
    links = CR.parent_links(lens, records, built['cls'])
    contained, dropped = built['contained'], built['dropped']
    best = {}
    for i, (rec, c) in enumerate(zip(records, built['cls'])):
        if c not in (R.A_TO_B, R.B_TO_A):
            continue
        for d, other in ((rec[0], rec[1]), (rec[1], rec[0])):
            if dropped[d] and not contained[other] and not dropped[other] and (d not in best or rec[7] > records[best[d]][7]):
                best[d] = i
    for d, i in best.items():
        a, b, strand, a_beg, _, b_beg, _, _, _ = records[i]
        assert d not in links                                 # a dropped read is never contained
        if d == a:
            delta = b_beg - a_beg
            links[d] = (b, strand, delta if strand == 0 else lens[b] - delta - lens[a])
        else:
            links[d] = (a, strand, a_beg - b_beg)
    return links


def place(lens, records, built):
    """One ``(unitig, rev, pos, root, depth)`` per read, as ``consensus_ref.place`` with the links above."""
    lens = [int(x) for x in lens]
    records = [tuple(int(x) for x in r) for r in records]
    links = parent_links(lens, records, built)
    first = {}
    for u, (fm, _, n, _, _) in enumerate(built['unitigs']):
        for v, _, off in built['members'][fm:fm + n]:
            first.setdefault(v >> 1, (u, v & 1, off))
    out = []
    for r in range(len(lens)):
        chain, x, seen = [], r, set()
        while x in links and x not in seen:
            seen.add(x)
            chain.append(x)
            x = links[x][0]
        if x in links or x not in first:
            out.append(CR.UNPLACED)
            continue
        cur, on = first[x], x
        for c in reversed(chain):
            p, rel, off = links[c]
            assert p == on
            cur, on = CR.compose(cur, lens[p], (rel, off), lens[c]), c
        out.append((cur[0], cur[1], cur[2], x, len(chain)))
    return out
