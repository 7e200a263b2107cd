"""Dense numpy reference of minimizer sampling (include/pw_kmers.h, THE SAMPLED TABLE; pw_overlap_all_pairs_sampled) -- TEST
INFRASTRUCTURE, never the product path.

Built on tests/kmer_ref.py.  The definition is restated, not shared with the device: the order values from the keys of
kmer_ref (the reverse complement of a k-mer from the reversed reverse-strand keys), the selection once by brute force over
every window and once by the lg / rg rule, the table with rc(read) MATERIALISED for strand 1 -- its rows are the selected
positions of rc(read) under its own order values, so the mirror symmetry the device relies on is checked, not assumed -- and the
join as kmer_ref.capped_join restricted to the selected rows, with the cap counted on the sampled table.
"""
import collections

import numpy as np

from tests import kmer_ref as KR


def mix(x):
    """The 64-bit bijection of the definition, on uint64 arrays (numpy wraps mod 2^64)."""
    x = np.asarray(x, np.uint64)
    with np.errstate(over='ignore'):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def mix_int(x):
    """The same on one Python integer (no numpy arithmetic): the check of `mix`."""
    m = (1 << 64) - 1
    z = (x + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def revcomp(read, comp):
    return np.asarray(comp, np.uint8)[np.asarray(read, np.uint8)[::-1]]


def order_values(read, k, L, canonical=False, comp=None):
    """h(p) for every position of `read`: mix(x(p)), or mix(min(x(p), x'(p))) with x'(p) the key of the reverse complement of
    the k-mer at p -- the k-mer of rc(read) at n - 1 - p."""
    x = KR.forward_keys(read, k, L)
    if canonical and len(x):
        x = np.minimum(x, KR.reverse_keys(read, k, L, comp)[::-1])
    return mix(x)


def select_brute(h, w):
    """Flags of the positions that attain the minimum of some window of min(w, n) consecutive positions."""
    n = len(h)
    sel = np.zeros(n, bool)
    if n == 0:
        return sel
    ww = min(w, n)
    for s in range(n - ww + 1):
        win = h[s:s + ww]
        sel[s:s + ww] |= win == win.min()
    return sel


def select_rule(h, w):
    """The same by the rule: lg / rg = the consecutive positions left / right of p with h >= h(p), stopping at the ends of the
    read and at ww - 1; selected exactly when lg + rg + 1 >= ww."""
    n = len(h)
    sel = np.zeros(n, bool)
    ww = min(w, n)
    for p in range(n):
        lg = 0
        while lg < ww - 1 and p - lg - 1 >= 0 and h[p - lg - 1] >= h[p]:
            lg += 1
        rg = 0
        while rg < ww - 1 and p + rg + 1 < n and h[p + rg + 1] >= h[p]:
            rg += 1
        sel[p] = lg + rg + 1 >= ww
    return sel


def selected(read, k, L, w, canonical=False, comp=None):
    """The selected positions of `read`, ascending."""
    return np.flatnonzero(select_brute(order_values(read, k, L, canonical, comp), w))


def _strand_rows(reads, k, L, w, strands, comp):
    """Per strand and read: (positions, keys) of the selected rows; strand 1 from the materialised rc(read)."""
    canonical = strands != '+'
    out = []
    for strand in ((0, 1) if canonical else (0,)):
        per_read = []
        for read in reads:
            seq = revcomp(read, comp) if strand else np.asarray(read, np.uint8)
            pos = selected(seq, k, L, w, canonical, comp)
            per_read.append((pos, KR.forward_keys(seq, k, L)[pos] if len(pos) else np.zeros(0, np.uint64)))
        out.append(per_read)
    return out


def table(reads, k, L, w, strands='+', comp=None):
    """(keys, hits) of the sampled table in table order, as kmer_ref.table."""
    keys, hits = [np.zeros(0, np.uint64)], [np.zeros(0, np.uint64)]
    for strand, per_read in enumerate(_strand_rows(reads, k, L, w, strands, comp)):
        for r, (pos, kk) in enumerate(per_read):
            keys.append(kk)
            hits.append((np.uint64(r) << np.uint64(32)) | np.uint64(strand * KR.STRAND_BIT) | pos.astype(np.uint64))
    keys, hits = np.concatenate(keys), np.concatenate(hits)
    order = np.lexsort((hits & np.uint64(0x7fffffff), hits >> np.uint64(32), (hits >> np.uint64(31)) & np.uint64(1), keys))
    return keys[order], hits[order]


def counts(reads, k, L, w, strands='+', comp=None):
    u, c = np.unique(table(reads, k, L, w, strands, comp)[0], return_counts=True)
    return u.astype(np.uint64), c.astype(np.uint32)


def read_starts(reads, k, L, w, strands='+', comp=None):
    """The sampled forward rows before every read (len(reads) + 1 entries)."""
    fwd = _strand_rows(reads, k, L, w, strands, comp)[0]
    return np.concatenate([[0], np.cumsum([len(pos) for pos, _ in fwd])]).astype(np.int64)


def occurrences(reads, k, L, w, strands='+', comp=None):
    """count(key) of every sampled forward row in (read, pos) order, counted over the sampled table."""
    u, c = counts(reads, k, L, w, strands, comp)
    fk = np.concatenate([np.zeros(0, np.uint64)] + [kk for _, kk in _strand_rows(reads, k, L, w, strands, comp)[0]])
    return c[np.searchsorted(u, fk)].astype(np.uint32) if len(fk) else np.zeros(0, np.uint32)


def num_positions(reads, k):
    return int(sum(max(len(r) - k + 1, 0) for r in reads))


SampledJoin = collections.namedtuple('SampledJoin', 'pairs stats')


def sampled_join(reads, k, L, w, max_occ=0, strands='+', comp=None, rank=0, world=1):
    """kmer_ref.capped_join restricted to the selected rows.  `pairs`: OrderedDict (a, b, strand) -> the diagonals of the seeds
    between two selected rows in table order (k-mer, then i, then j), for a < b, a % world == rank, ascending (a, b, strand),
    pairs without a surviving seed left out.  The cap (0 or None: none) is counted on the sampled table: over both strands
    unless strands == '+'.  `stats`: positions, sampled, density and, under a cap, the five counters of pw_overlap_cap_stats."""
    rows = _strand_rows(reads, k, L, w, strands, comp)
    u, c = counts(reads, k, L, w, '+' if strands == '+' else 'both', comp)
    masked = u[c > max_occ] if max_occ else np.zeros(0, np.uint64)
    pairs = collections.OrderedDict()
    dropped = 0
    for a in range(len(reads)):
        if a % world != rank:
            continue
        pa, ka = rows[0][a]
        for b in range(a + 1, len(reads)):
            for strand in {'+': (0,), '-': (1,), 'both': (0, 1)}[strands]:
                pb, kb = rows[strand][b]
                key, i, j = KR._seed_rows(ka, kb)
                if len(key) == 0:
                    continue
                d = pa[i].astype(np.int64) - pb[j].astype(np.int64)
                kept = d[~np.isin(key, masked)]
                dropped += len(d) - len(kept)
                if len(kept):
                    pairs[(a, b, strand)] = kept
    positions, sampled = num_positions(reads, k), int(sum(len(pos) for pos, _ in rows[0]))
    stats = dict(positions=positions, sampled=sampled, density=sampled / positions if positions else float('nan'))
    if max_occ:
        stats.update(entries=int(c.sum()), masked_entries=int(c[c > max_occ].sum()), distinct_masked=int(len(masked)),
                     seeds_kept=int(sum(len(d) for d in pairs.values())), seeds_dropped=int(dropped))
    return SampledJoin(pairs, stats)


# ---- the fixtures of the GPU tests ---------------------------------------------------------------------------------------
def edge_reads(L, k, w, comp=None, seed=0):
    """At most 16 reads of at most 2 000 letters for window w: an empty read and one shorter than k; reads with n = 1, w - 1, w
    and w + 1 positions next to each other (halos cross read boundaries); reads with 255, 256, 257 and 256 + w - 1 positions
    (the tile edges); a homopolymer of the last letter (the largest key) and a short one of letter 0; a period-3 tandem repeat; a stretch followed by its own reverse complement under `comp`
    (default: the DNA complement for L = 4, else the identity -- a plain palindrome)."""
    rng = np.random.default_rng(seed * 1000 + w)

    def rnd(n_pos):
        return rng.integers(0, L, n_pos + k - 1).astype(np.uint8) if n_pos > 0 else np.zeros(0, np.uint8)

    reads = [np.zeros(0, np.uint8), rng.integers(0, L, k - 1).astype(np.uint8)]
    reads += [rnd(n) for n in (1, max(w - 1, 1), w, w + 1)]
    reads += [rnd(n) for n in (255, 256, 257, 256 + w - 1)]
    reads.append(np.full(90 + k - 1, L - 1, np.uint8))                                  # homopolymer
    reads.append(np.resize(np.array([0, L - 1, min(1, L - 1)], np.uint8), 120 + k - 1))     # period 3
    half = rng.integers(0, L, 60 + k).astype(np.uint8)
    if comp is None:
        comp = KR.DNA_COMPLEMENT if L == 4 else np.arange(L, dtype=np.uint8)
    reads.append(np.concatenate([half, revcomp(half, comp)]))                          # reverse-palindromic
    reads.append(np.zeros(k + 4, np.uint8))                                            # key 0, five times
    assert len(reads) <= 16 and max(len(r) for r in reads) <= 2000
    return reads


GUARANTEE_K, GUARANTEE_W, GUARANTEE_L = 8, 10, 4


def guarantee_reads(seed=7):
    """10 reads of 400 letters cut error-free from one 1 500-letter random genome, every other one reverse-complemented.
    Returns (reads, starts, flipped)."""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, 1500).astype(np.uint8)
    starts = np.sort(rng.integers(0, 1100, 10))
    flipped = [bool(q % 2) for q in range(10)]
    reads = [revcomp(genome[s:s + 400], KR.DNA_COMPLEMENT) if f else genome[s:s + 400].copy() for s, f in zip(starts.tolist(), flipped)]
    return reads, starts.tolist(), flipped


def guarantee_truth(starts, flipped, min_overlap, length=400):
    """{(a, b): (strand, true diagonal)} for a < b whose genome intervals overlap by at least min_overlap letters.  The pair is
    on strand 1 when exactly one read is flipped.  The diagonal is i - j' for matching letters i of S = reads[a] and j' of T =
    reads[b] (strand 0) or rc(reads[b]) (strand 1): with g = a genome position, an unflipped read has index g - start and a
    flipped one length - 1 - (g - start); T is in the orientation of S."""
    out = {}
    for a in range(len(starts)):
        for b in range(a + 1, len(starts)):
            if length - abs(starts[a] - starts[b]) < min_overlap:
                continue
            # T is reads[b] when both have the same orientation, rc(reads[b]) otherwise: either way T runs as S does
            d = (starts[b] - starts[a]) if not flipped[a] else (starts[a] - starts[b])
            out[(a, b)] = (int(flipped[a] != flipped[b]), d)
    return out
