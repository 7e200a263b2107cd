"""CPU oracle of the consensus layout: a direct restatement of the contract in include/pw_consensus.h in plain Python.
Placements follow every containment chain link by link with a visited set and compose from the root down (the device
doubles pointers and composes in another order: the operation is associative); tasks, the padded contig starts and the
arena bytes are written out as the header states them.  Records are the tuples of tests/graph_ref.py, ``built`` is the
dict ``graph_ref.build`` returns; results are plain tuples in the field order of the C records."""
import numpy as np

A_CONTAINED, B_CONTAINED = 3, 4
UNPLACED = (-1, 0, 0, 0, 0)


def parent_links(lens, records, cls):
    """``{child: (parent, rel, off)}`` from the parent record of every contained read: the largest n_match, a tie to the lowest
    record index; the four-row table."""
    best = {}
    for i, (rec, c) in enumerate(zip(records, cls)):
        if c not in (A_CONTAINED, B_CONTAINED):
            continue
        child = rec[0] if c == A_CONTAINED else rec[1]
        if child not in best or rec[7] > records[best[child]][7]:
            best[child] = i
    links = {}
    for child, i in best.items():
        a, b, strand, a_beg, _, b_beg, _, _, _ = records[i]
        if cls[i] == A_CONTAINED:
            delta = b_beg - a_beg
            links[child] = (b, strand, delta if strand == 0 else lens[b] - delta - lens[a])
        else:
            links[child] = (a, strand, a_beg - b_beg)
    return links


def compose(parent_place, lp, child, lc):
    """(F, rel_p, off_p) of a read of lp letters, and (rel_c, off_c) of a read of lc letters on it."""
    F, rel_p, off_p = parent_place
    rel_c, off_c = child
    if rel_p == 0:
        return (F, rel_c, off_p + off_c)
    return (F, rel_c ^ 1, off_p + lp - off_c - lc)


def place(lens, records, built):
    """One ``(unitig, rev, pos, root, depth)`` per read."""
    lens = [int(x) for x in lens]
    records = [tuple(int(x) for x in r) for r in records]
    links = parent_links(lens, records, built['cls'])
    first = {}
    for u, (fm, _, n, _, _) in enumerate(built['unitigs']):
        for v, _, off in built['members'][fm:fm + n]:
            first.setdefault(v >> 1, (u, v & 1, off))            # (members are visited in ascending member index)
    out = []
    for r in range(len(lens)):
        chain, x, seen = [], r, set()
        while x in links and x not in seen:
            seen.add(x)
            chain.append(x)
            x = links[x][0]
        if x in links or x not in first:                         # a cycle, or a root that is no member
            out.append(UNPLACED)
            continue
        cur, on = first[x], x                                    # the placement of read `on`
        for c in reversed(chain):
            p, rel, off = links[c]
            assert p == on
            cur, on = compose(cur, lens[p], (rel, off), lens[c]), c
        out.append((cur[0], cur[1], cur[2], x, len(chain)))
    return out


def contig_starts(unitigs):
    cs = [0]
    for u in unitigs:
        if u[1] >= 1 << 31:
            raise ValueError('a contig has 2**31 letters or more')
        cs.append((cs[-1] + u[1] + 3) & ~3)
    return cs


def tasks(lens, places, unitigs, slack, drift):
    """``(tasks, cstart, arena_bytes)``; a task is ``(col0, mut_off, read, win_len, dmin, dmax, rev, 0)``."""
    cs = contig_starts(unitigs)
    at = (cs[-1] + 15) & ~15
    out = []
    for r, (u, rev, pos, _, _) in enumerate(places):
        l = int(lens[r])
        if u < 0 or l <= 0:
            continue
        length = unitigs[u][1]
        if not max(pos, 0) < min(pos + l, length):
            continue
        radius = slack + int(float(l) * drift)
        lo = max(0, pos - radius) & ~3
        hi = min(length, pos + l + radius)
        d0 = pos - lo
        out.append((cs[u] + lo, at, r, hi - lo, max(d0 - radius, -l), min(d0 + radius, hi - lo), rev, 0))
        at += (l + 15) // 16 * 16 + 16
    return out, cs, at + 16


def oriented(read, rev, complement=None):
    r = np.asarray(read, np.uint8)
    if not rev:
        return r.copy()
    r = r[::-1].copy()
    if complement is not None:
        comp = np.asarray(complement, np.uint8)
        inside = r < len(comp)
        r[inside] = comp[r[inside]]
    return r


def arena(reads, contigs, task_list, cstart, arena_bytes, complement=None):
    """The consensus arena's bytes: ``contigs`` are the draft letters in unitig order."""
    out = np.zeros(arena_bytes, np.uint8)
    out[:cstart[-1]] = 255
    for u, c in enumerate(contigs):
        out[cstart[u]:cstart[u] + len(c)] = np.asarray(c, np.uint8)
    for _, mut_off, r, _, _, _, rev, _ in task_list:
        o = oriented(reads[r], rev, complement)
        out[mut_off:mut_off + len(o)] = o
    return out
