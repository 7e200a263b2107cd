"""Minimizer sampling on config 4's shape, on one MI355X: R synthetic 5 kb reads at 25x coverage, k = 16.

    python tests/micro/minimizer_bench.py [n_reads] [wordlen] [--plus-only]

For both strand settings ('+' on the reads as cut; 'both' with every other read reverse-complemented, so that half of the
true overlaps are minus pairs) and window None, 5, 10 and 20:
  * rows: the forward rows of the index, beside the positions and the 2 / (w + 1) the density should come to on this
    random-genome input;
  * build: device ms of the k-mer table's build (kmers.KmerIndex: HIP events; the sampled build includes its wait for the row
    count);
  * all pairs: device ms of overlap.raw_all_pairs, seeds kept, pairs listed;
  * recall: of the true overlaps longer than 500 bases that the unsampled call of the same run lists (on the right strand), the
    share this window lists -- and the share whose band [d_best - r_best, d_best + r_best], widened by 150 for the drift of the
    reads' indels, holds the difference of the reads' starts.
Device ms after a warm-up call, calls repeated 5 to 12 times (until a second at the fastest call's pace): min / median / max.
Output: stdout (committed as profiles/minimizer_bench.txt).
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from biseqt_amd import synth                            # noqa: E402
from biseqt_amd.kmers import kmer_spectrum              # noqa: E402
from biseqt_amd.overlap import raw_all_pairs            # noqa: E402
from biseqt_amd.sequence import Alphabet                # noqa: E402

COMP = np.array([3, 2, 1, 0], np.uint8)
READ_LEN, COV, MIN_OVERLAP, DRIFT = 5000, 25, 500, 150


def config4_reads(R):
    """The read set of tests/micro/overlap_all_bench.py, with the reads' starts."""
    rng = synth.rng_for(4)
    G = R * READ_LEN // COV
    g = synth.rand_seqs(rng, 1, G)[0]
    starts = rng.integers(0, G - READ_LEN, R)
    return [np.asarray(synth.mutate(rng, g[s:s + READ_LEN], .05, .025, .025), np.uint8) for s in starts], starts


def repeated(call, budget_ms=1000., least=5, most=12):
    """call() -> device ms; after one warm-up, repeated at least `least` times and until `budget_ms` at the pace of the fastest
    call, `most` times at the most: (min, median, max, calls) and the last call's result.  (The fastest call's pace: one call
    in a few reports seconds where its seed buffers are first allocated inside the timed region -- profiles/
    kmer_spectrum_bench.txt shows the same -- and must not end the series.  `most`: every call also packs and uploads 250 MB
    of reads on the host, which is not what is measured.)"""
    call()
    ms, out = [], None
    while len(ms) < least or (min(ms) * len(ms) < budget_ms and len(ms) < most):
        out = call()
        ms.append(out[0])
    return (min(ms), float(np.median(ms)), max(ms), len(ms)), out


def truth(pairs, flags, recs, starts, flipped, R):
    """Of the listed pairs: which are true overlaps > MIN_OVERLAP on the right strand (their keys a * R + b), and which of those
    hold the start difference in their band."""
    a, b = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    ov = np.minimum(starts[a], starts[b]) + READ_LEN - np.maximum(starts[a], starts[b])
    true = (ov > MIN_OVERLAP) & ((flipped[a] != flipped[b]) == (flags == 1))
    d_true = np.where(flipped[a], starts[a] - starts[b], starts[b] - starts[a])      # T runs as S does (tests/minimizer_ref.py)
    held = np.abs(recs['d_best'].astype(np.int64) - d_true) <= recs['r_best'].astype(np.int64) + DRIFT
    key = a * R + b
    return key[true], key[true & held]


def main():
    args = [x for x in sys.argv[1:] if not x.startswith('--')]
    R = int(args[0]) if args else 50000
    k = int(args[1]) if len(args) > 1 else 16
    A = Alphabet('ACGT')
    t0 = time.perf_counter()
    reads, starts = config4_reads(R)
    print('%d reads of 5 kb (25x), k = %d; reads generated in %.1f s' % (R, k, time.perf_counter() - t0))
    raw_all_pairs(reads[:50], k, 4, .2, .9, strands='both', complement=COMP, minimizer_window=5)        # code objects
    for strands in ('+',) if '--plus-only' in sys.argv else ('+', 'both'):
        flipped = (np.arange(R) % 2 == 1) if strands == 'both' else np.zeros(R, bool)
        rs = [COMP[r[::-1]] if f else r for r, f in zip(reads, flipped)]
        cap = min(R * (R - 1) // 2 * (2 if strands == 'both' else 1), 1 << (25 if strands == 'both' else 24))
        print("strands '%s'%s" % (strands, ': every other read reverse-complemented' if strands == 'both' else ''))
        base = None
        for w in (None, 5, 10, 20):
            with kmer_spectrum(rs, k, A, strands=strands, complement=COMP, window=w) as idx:
                def build():
                    idx._dirty = True
                    idx._lib.pw_kmers_num_distinct(idx._table())           # waits for the build: last_ms is the build's
                    return (idx.last_ms,)
                b, _ = repeated(build)
                rows, positions, entries = int(idx.read_starts[-1]), idx.num_positions, idx.num_entries
            stats = {}

            def join():
                if strands == '+':                                         # (window None: the call of overlap_all_bench.py)
                    p, r, ms = raw_all_pairs(rs, k, 4, .2, .9, max_pairs=cap, minimizer_window=w, stats=stats)
                    return ms, p, np.zeros(len(p), np.uint8), r
                p, f, r, ms = raw_all_pairs(rs, k, 4, .2, .9, max_pairs=cap, strands=strands, complement=COMP, minimizer_window=w,
                                            stats=stats)
                return ms, p, f, r
            j, (_, pairs, flags, recs) = repeated(join)
            listed, held = truth(pairs, flags, recs, starts, flipped, R)
            if base is None:
                base = (listed, held)
            print('  window %-4s rows %11d of %d positions = %.4f (2 / (w + 1) = %s), table rows %d'
                  % (w, rows, positions, rows / positions, '%.4f' % (2. / (w + 1)) if w else '1', entries))
            print('    build     %8.2f / %8.2f / %8.2f ms (min / median / max of %d calls)' % b)
            print('    all pairs %8.2f / %8.2f / %8.2f ms (min / median / max of %d calls): %d seeds kept, %d pairs listed'
                  % (j + (int(recs['n_seeds'].sum()), len(pairs))))
            print('    true overlaps > %d bases listed: %d = %.4f of the unsampled call\'s %d; with the start difference in the band: '
                  '%d = %.4f of its %d' % (MIN_OVERLAP, len(listed), len(np.intersect1d(listed, base[0])) / max(len(base[0]), 1),
                                           len(base[0]), len(held), len(np.intersect1d(held, base[1])) / max(len(base[1]), 1), len(base[1])))
            if stats:
                print('    stats %s' % stats)


if __name__ == '__main__':
    main()
