"""CPU oracle of the overlap graph: a direct restatement of the contract in include/pw_graph.h in plain Python, with dict
look-ups and no cleverness.  Records are tuples ``(a, b, strand, a_beg, a_end, b_beg, b_end, n_match, n_ops)``; every
result is a list of plain tuples in the field order of the C records, so a test compares ``==`` after ``.tolist()``."""
NONE, WEAK, INTERNAL, A_CONTAINED, B_CONTAINED, A_TO_B, B_TO_A = range(7)
REDUCED, REMOVED, CHAIN = 1, 2, 4
DEFAULTS = dict(max_hang=1000, int_frac=.8, min_overlap=0, min_identity=0., fuzz=10)


def classify(rec, lens, max_hang, int_frac, min_overlap, min_identity):
    a, b, _, a_beg, a_end, b_beg, b_end, n_match, n_ops = rec
    la, lb = lens[a], lens[b]
    if n_ops == 0:
        return NONE
    if min(a_end - a_beg, b_end - b_beg) < min_overlap or float(n_match) < min_identity * float(n_ops):
        return WEAK
    ext = min(a_beg, b_beg) + min(la - a_end, lb - b_end)
    span = max(a_end - a_beg, b_end - b_beg)
    x, y = float(max_hang), float(span) * int_frac
    if float(ext) > (y if y < x else x):
        return INTERNAL
    if a_beg <= b_beg and la - a_end <= lb - b_end:
        return A_CONTAINED
    if a_beg >= b_beg and la - a_end >= lb - b_end:
        return B_CONTAINED
    return A_TO_B if a_beg > b_beg else B_TO_A


def build(lens, records, max_hang=1000, int_frac=.8, min_overlap=0, min_identity=0., fuzz=10):
    """Returns a dict: ``cls`` (one per record), ``contained`` (one per read), ``arcs`` (v, w, len, ol, src, flags) sorted,
    ``rows`` (2 * n_reads + 1), ``unitigs`` (first_member, length, n_members, head, circular), ``members`` (vertex, advance,
    offset)."""
    lens = [int(x) for x in lens]
    records = [tuple(int(x) for x in r) for r in records]
    n_reads, V = len(lens), 2 * len(lens)
    keys = set()
    for r in records:
        if r[:3] in keys:
            raise ValueError('duplicate overlap key %r' % (r[:3],))
        keys.add(r[:3])
    cls = [classify(r, lens, max_hang, int_frac, min_overlap, min_identity) for r in records]
    contained = [0] * n_reads
    for r, c in zip(records, cls):
        if c == A_CONTAINED:
            contained[r[0]] = 1
        elif c == B_CONTAINED:
            contained[r[1]] = 1
    gen = []
    for i, (r, c) in enumerate(zip(records, cls)):
        a, b, strand, a_beg, a_end, b_beg, b_end, _, _ = r
        if c not in (A_TO_B, B_TO_A) or contained[a] or contained[b]:
            continue
        la, lb = lens[a], lens[b]
        va, vb = 2 * a, 2 * b + strand
        if c == A_TO_B:
            gen.append([va, vb, a_beg - b_beg, a_end - a_beg, i, 0])
            gen.append([vb ^ 1, va + 1, (lb - b_end) - (la - a_end), b_end - b_beg, i, 0])
        else:
            gen.append([vb, va, b_beg - a_beg, b_end - b_beg, i, 0])
            gen.append([va + 1, vb ^ 1, (la - a_end) - (lb - b_end), a_end - a_beg, i, 0])
    assert all(arc[2] >= 1 for arc in gen)
    order = sorted(range(len(gen)), key=lambda g: (gen[g][0], gen[g][2], g))
    arcs = [gen[g] for g in order]
    where = {g: s for s, g in enumerate(order)}
    rows = [0] * (V + 1)
    for arc in arcs:
        rows[arc[0] + 1] += 1
    for v in range(V):
        rows[v + 1] += rows[v]
    # transitive reduction: every pair of arcs v -> w, w -> x against every arc v -> x
    leaving, between = {}, {}
    for s, arc in enumerate(arcs):
        leaving.setdefault(arc[0], []).append(s)
        between.setdefault((arc[0], arc[1]), []).append(s)
    for v, row in leaving.items():
        for s1 in row:
            w, len1 = arcs[s1][1], arcs[s1][2]
            for s2 in leaving.get(w, []):
                x, len2 = arcs[s2][1], arcs[s2][2]
                if x == w:
                    continue
                for s3 in between.get((v, x), []):
                    if len1 + len2 <= arcs[s3][2] + fuzz:
                        arcs[s3][5] |= REDUCED
    reduced = [arc[5] & REDUCED for arc in arcs]
    for s, g in enumerate(order):
        if reduced[s] or reduced[where[g ^ 1]]:
            arcs[s][5] |= REMOVED
    # unitigs
    out = [0] * V
    for arc in arcs:
        if not arc[5] & REMOVED:
            out[arc[0]] += 1
    succ, pred, adv = {}, {}, {}
    for arc in arcs:
        v, w = arc[0], arc[1]
        if not arc[5] & REMOVED and out[v] == 1 and out[w ^ 1] == 1 and w != v and w != v ^ 1:
            arc[5] |= CHAIN
            assert v not in succ and w not in pred
            succ[v], pred[w], adv[v] = w, v, arc[2]
    live = [v for v in range(V) if not contained[v >> 1]]
    seen, comps = set(), []
    for v in live:
        if v in seen:
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
        seen.update(path)
        comps.append((path, circular))
    unitigs, members = [], []
    for path, circular in sorted((c for c in comps if min(c[0]) % 2 == 0), key=lambda c: c[0][0]):
        first, off = len(members), 0
        for k, v in enumerate(path):
            step = adv[v] if (k + 1 < len(path) or circular) else lens[v >> 1]
            members.append((v, step, off))
            off += step
        unitigs.append((first, off, len(path), path[0], int(circular)))
    return dict(cls=cls, contained=contained, arcs=[tuple(a) for a in arcs], rows=rows, unitigs=unitigs, members=members)


def oriented(reads, v, complement=None):
    """The letters of vertex ``v``: read ``v >> 1`` as stored, or reverse-complemented (a letter outside the table stays)."""
    r = [int(c) for c in reads[v >> 1]]
    if not v & 1:
        return r
    return [(int(complement[c]) if complement is not None and c < len(complement) else c) for c in reversed(r)]


def contigs(reads, unitigs, members, complement=None):
    """The contig letters, a list of lists of ints, in unitig order."""
    out = []
    for first, _, n, _, _ in unitigs:
        letters = []
        for v, step, _ in members[first:first + n]:
            letters.extend(oriented(reads, v, complement)[:step])
        out.append(letters)
    return out
