"""The k-mer table and the occurrence cap on config 4's read set, on one MI355X: R synthetic 5 kb reads at 25x coverage.

    python tests/micro/kmer_spectrum_bench.py [n_reads] [wordlen] [--no-overlap] [--no-host]

  * build and spectrum of the whole read set's table (device ms from HIP events: after a warm-up, repeated until the timed
    calls add up to at least a second; min / median / max) beside np.unique(return_counts=True) on the host for the same
    keys;
  * overlap_all_pairs' device pass (raw_all_pairs) on that set, and on a copy with a 300-letter repeat planted in 20 % of the
    reads, at max_kmer_occ in {None, 1000, 100}, with the cap's counters.
Output: stdout (committed as profiles/kmer_spectrum_bench.txt).
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


def config4_reads(R, read_len=5000, cov=25):
    """The read set of tests/micro/overlap_all_bench.py."""
    rng = synth.rng_for(4)
    G = R * read_len // cov
    g = synth.rand_seqs(rng, 1, G)[0]
    starts = rng.integers(0, G - read_len, R)
    return [synth.mutate(rng, g[s:s + read_len], .05, .025, .025) for s in starts]


def with_repeat(reads, length=300, share=.2, seed=1):
    """A copy with one `length`-letter repeat written into `share` of the reads (a transposon: every copy identical)."""
    rng = np.random.default_rng(seed)
    rep = rng.integers(0, 4, length).astype(np.uint8)
    out = [np.array(r, np.uint8) for r in reads]
    for r in rng.choice(len(out), int(len(out) * share), replace=False):
        if len(out[r]) > length:
            at = int(rng.integers(0, len(out[r]) - length))
            out[r][at:at + length] = rep
    return out


def timed(call, ms_of, budget_ms=1000.):
    """Device ms of repeated calls after one warm-up, until they add up to budget_ms: (min, median, max, calls)."""
    call()
    ms = []
    while sum(ms) < budget_ms:
        call()
        ms.append(ms_of())
    return min(ms), float(np.median(ms)), max(ms), len(ms)


def host_keys(reads, k):
    out = []
    for r in reads:
        r = np.asarray(r, np.uint64)
        n = len(r) - k + 1
        if n <= 0:
            continue
        key = np.zeros(n, np.uint64)
        for t in range(k):
            key = key * np.uint64(4) + r[t:t + n]
        out.append(key)
    return np.concatenate(out)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    R = int(args[0]) if args else 50000
    k = int(args[1]) if len(args) > 1 else 16
    A = Alphabet('ACGT')
    t0 = time.perf_counter()
    reads = config4_reads(R)
    print('%d reads of 5 kb (25x), k = %d; reads generated in %.1f s' % (R, k, time.perf_counter() - t0))
    for strands in ('+', 'both'):
        with kmer_spectrum(reads, k, A, strands=strands, complement=[('A', 'T'), ('C', 'G')]) as idx:
            distinct = []

            def build():
                idx._dirty = True                           # rebuild the device table from the same reads ...
                distinct[:] = [idx._lib.pw_kmers_num_distinct(idx._table())]     # ... and wait for it: last_ms is the build's
            b = timed(build, lambda: idx.last_ms)
            s = timed(lambda: idx.spectrum(64), lambda: idx.last_ms)
            o = timed(lambda: idx.all_occurrences(), lambda: idx.last_ms)
            hist = idx.spectrum(64)
            n, d = idx.num_entries, int(distinct[0])
            print("strands '%s': %d rows, %d distinct" % (strands, n, d))
            print('  build        %8.2f / %8.2f / %8.2f ms (min / median / max of %d calls) = %.0f M rows/s' % (b + (n / b[1] / 1e3,)))
            print('  spectrum(64) %8.3f / %8.3f / %8.3f ms (%d calls)' % s)
            print('  occurrences  %8.2f / %8.2f / %8.2f ms (%d calls, kernel only)' % o)
            print('  hist[1..8] = %s, hist[64] (count >= 64) = %d' % (hist[1:9].tolist(), int(hist[64])))
            if strands == '+' and '--no-host' not in sys.argv:
                keys = host_keys(reads, k)
                t1 = time.perf_counter()
                u, c = np.unique(keys, return_counts=True)
                t2 = time.perf_counter()
                hk, hc = idx.counts()
                assert np.array_equal(hk, u) and np.array_equal(hc, c.astype(np.uint32))
                print('  host: np.unique(return_counts=True) of the same %d keys %.0f ms (equal keys and counts)' % (len(keys), (t2 - t1) * 1e3))
    if '--no-overlap' in sys.argv:
        return
    cap = min(R * (R - 1) // 2, 1 << 23)
    raw_all_pairs(reads[:50], k, 4, .2, .9, max_kmer_occ=100)
    for name, rs in (('config 4', reads), ('config 4 + a 300-letter repeat in 20 % of the reads', with_repeat(reads))):
        print(name)
        for occ in (None, 1000, 100):
            stats = {}
            try:
                ms = []
                while len(ms) < 3 or sum(ms) < 1000.:
                    pairs, recs, one = raw_all_pairs(rs, k, 4, .2, .9, max_pairs=cap, max_kmer_occ=occ, stats=stats)
                    ms.append(one)
                print('  max_kmer_occ=%-5s device %8.1f / %8.1f / %8.1f ms (min / median / max of %d calls), %d candidate pairs, %d seeds  %s'
                      % (occ, min(ms), float(np.median(ms)), max(ms), len(ms), len(pairs), int(recs['n_seeds'].sum()), stats or ''))
            except RuntimeError as e:
                print('  max_kmer_occ=%-5s refused: %s  %s' % (occ, e, stats or ''))


if __name__ == '__main__':
    main()
