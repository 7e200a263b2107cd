"""CIGARs on the device (pw_cigar.hip) beside what they stand next to.

    python tests/micro/cigar_bench.py [--pairs N] [--runs R] [--map-repeats K] [--no-map]
    python tests/micro/cigar_bench.py --default-only [--root CHECKOUT] [--label NAME]

Part 1, two solved batches -- BASELINE config 2 (10 000 pairs of 2 kb, band radius 200, B_LOCAL, 1 / -3 / -5 / -2) and the
batch pipeline.map_queries builds at the read-mapping shape of tests/micro/blot_many_bench.py (10 000 queries of 250 letters
against 100 kb) -- R runs after three untimed ones: device milliseconds of pw_batch_cigars (count + offsets + the read-back of
the 8-byte total + write: the events span the whole call, the blocking read included), of pw_batch_pack_transcripts and of
pw_batch_summarize, each between two HIP events recorded around the call on the default stream.  Medians and minima, and the
bytes a caller moves to the host: runs + offsets against packed ops + offsets.

Part 2, the read-mapping shape: host wall seconds of pipeline.map_queries with alignments=True, with alignments=False and with
alignments=False, cigar='extended', interleaved, K calls each after one untimed call of each on 8 queries; the clocks end with
the results on the host.

--default-only times the default call alone (alignments=True, no cigar) and prints one line per call: the A/B of two
checkouts runs it once per checkout, alternating, with --root naming the checkout whose package is imported."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _import_from(root):
    sys.path.insert(0, root)
    import biseqt_amd                                   # noqa: F401  (this checkout's, or --root's)
    sys.path.insert(0, HERE)
    assert os.path.realpath(os.path.dirname(os.path.dirname(biseqt_amd.__file__))) == os.path.realpath(root), biseqt_amd.__file__


def hip_runtime():
    """The HIP runtime pwlib.so is bound to (the one mapped into this process), for the events."""
    from biseqt_amd import _pwlib as W
    W.load()
    with open('/proc/self/maps') as f:
        paths = sorted({ln.split()[-1] for ln in f if 'libamdhip64' in ln})
    hip = C.CDLL(paths[0])
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]
    return hip


class Events(object):
    def __init__(self, hip, n):
        self.hip, self.ev = hip, [C.c_void_p() for _ in range(n)]
        for e in self.ev:
            assert hip.hipEventCreate(C.byref(e)) == 0

    def record(self, k):
        assert self.hip.hipEventRecord(self.ev[k], None) == 0

    def ms(self, a, b):
        out = C.c_float()
        assert self.hip.hipEventSynchronize(self.ev[b]) == 0
        assert self.hip.hipEventElapsedTime(C.byref(out), self.ev[a], self.ev[b]) == 0
        return float(out.value)

    def close(self):
        for e in self.ev:
            self.hip.hipEventDestroy(e)


def stats(name, v, extra=''):
    print('%-52s median %8.4f ms   min %8.4f ms   (%d runs)%s' % (name, float(np.median(v)), min(v), len(v), extra), flush=True)


def kernels(b, what, runs):
    """The three readers of the op bytes on one solved batch."""
    from biseqt_amd.batch import cigar_of_transcript, cigar_strings
    ev = Events(hip_runtime(), 8)
    t = {k: [] for k in ('extended', 'classic', 'pack', 'summarize')}
    for r in range(3 + runs):
        b.traceback()
        ev.record(0); b._ck(b.lib.pw_batch_cigars(b.handle, 0, None), 'pw_batch_cigars'); ev.record(1)
        ev.record(2); b._ck(b.lib.pw_batch_cigars(b.handle, 1, None), 'pw_batch_cigars'); ev.record(3)
        ev.record(4); b.pack_transcripts(); ev.record(5)
        ev.record(6); b.summarize(); ev.record(7)
        b.sync()
        if r >= 3:
            for k, key in enumerate(('extended', 'classic', 'pack', 'summarize')):
                t[key].append(ev.ms(2 * k, 2 * k + 1))
    res = b.results()
    ops = int(np.maximum(res['tx_len'], 0).sum())
    ext, cla = b.cigars('extended'), b.cigars('classic')
    assert int((ext[0] >> 4).sum()) == int((cla[0] >> 4).sum()) == ops
    txs = b.transcripts(res)
    sample = list(range(0, b.n, max(1, b.n // 200)))
    strings = cigar_strings(*ext)
    assert all(strings[k] == cigar_of_transcript(txs[k]) for k in sample)
    n_tx = int((res['tx_len'] > 0).sum())
    print('%s; %s; %d ops in %d transcripts (%.0f per transcript); %d runs extended (%.1f per transcript), %d classic' %
          (what, b.kernel_name, ops, n_tx, ops / max(1, n_tx), len(ext[0]), len(ext[0]) / max(1, n_tx), len(cla[0])), flush=True)
    stats('pw_batch_cigars extended (count+offsets+read+write)', t['extended'])
    stats('pw_batch_cigars classic  (count+offsets+read+write)', t['classic'])
    stats('pw_batch_pack_transcripts (offsets + pack)', t['pack'])
    stats('pw_batch_summarize (k_tx_summary)', t['summarize'])
    off_bytes = 8 * (b.n + 1)
    print('bytes to the host: runs + offsets %d extended, %d classic; packed ops + offsets %d   (%.3f / %.3f of the packed ops)' %
          (4 * len(ext[0]) + off_bytes, 4 * len(cla[0]) + off_bytes, ops + off_bytes, (4 * len(ext[0]) + off_bytes) / (ops + off_bytes),
           (4 * len(cla[0]) + off_bytes) / (ops + off_bytes)), flush=True)
    ev.close()


def config2(n_pairs, runs):
    from biseqt_amd import synth
    from biseqt_amd.batch import BatchAligner
    origins, mutants = synth.pair_batch(2, n_pairs, 2000)
    with BatchAligner(list(zip(origins, mutants)), alnmode=1, alntype=1, alphabet_len=4, diag_range=(-200, 200), match_score=1,
                      mismatch_score=-3, go_score=-5, ge_score=-2) as b:
        b.solve()
        kernels(b, 'config 2: %d pairs of 2 kb, band radius 200, B_LOCAL' % n_pairs, runs)


def map_shape():
    import blot_many_bench as M
    sh = M.SHAPES['map']
    ref, queries = M.make('map', sh['queries'])
    return sh, ref, queries, (sh['K_min'], M.P_MIN, sh['wordlen'], M.G_MAX, M.SENS)


def mapping_batch(runs):
    """The batch map_queries aligns at the mapping shape, built again from its records (read 0 is the reference)."""
    from biseqt_amd import _pwlib as W
    from biseqt_amd.batch import BatchAligner, pack_reads
    from biseqt_amd.pipeline import map_queries
    sh, ref, queries, args = map_shape()
    mapped = map_queries(ref, queries, *args, alignments=False)
    arena, offs, lens = pack_reads([ref] + queries)
    pairs = [(0, 1 + q) for q, recs in enumerate(mapped) for _ in recs]
    bands = [rec['diag_range'] for recs in mapped for rec in recs]
    with BatchAligner.from_arena(arena, offs, lens, pairs, diag_ranges=bands, alphabet_len=4, alnmode=W.BANDED_MODE, alntype=W.B_LOCAL,
                                 match_score=1, mismatch_score=-3, go_score=-5, ge_score=-2) as b:
        b.solve()
        kernels(b, 'mapping shape: %d pairs of %d queries of %d against %d, B_LOCAL' % (len(pairs), len(queries), sh['qlen'], len(ref)), runs)


def mapping_walls(repeats):
    from biseqt_amd.pipeline import map_queries
    sh, ref, queries, args = map_shape()
    ways = (('alignments=True', dict(alignments=True)), ('alignments=False', dict(alignments=False)),
            ("alignments=False, cigar='extended'", dict(alignments=False, cigar='extended')))
    for _, kw in ways:
        map_queries(ref, queries[:8], *args, **kw)
    walls, got = {name: [] for name, _ in ways}, {}
    for _ in range(repeats):
        for name, kw in ways:
            t0 = time.perf_counter()
            got[name] = map_queries(ref, queries, *args, **kw)
            walls[name].append(time.perf_counter() - t0)
    for name, _ in ways:
        n_aln = sum(r['score'] is not None for recs in got[name] for r in recs)
        print('map_queries, %d queries of %d against %d, %-36s wall %s s   median %.4f   (%d alignments)'
              % (len(queries), sh['qlen'], len(ref), name, ' '.join('%.4f' % w for w in walls[name]), float(np.median(walls[name])), n_aln),
              flush=True)
    full, cg = got['alignments=True'], got["alignments=False, cigar='extended'"]
    from biseqt_amd.batch import cigar_of_transcript
    assert all((f['alignment'] is None and c['cigar'] is None) or c['cigar'] == cigar_of_transcript(f['alignment'].transcript)
               for fr, cr in zip(full, cg) for f, c in zip(fr, cr))


def default_only(label, repeats):
    from biseqt_amd.pipeline import map_queries
    sh, ref, queries, args = map_shape()
    map_queries(ref, queries[:8], *args)
    for _ in range(repeats):
        t0 = time.perf_counter()
        got = map_queries(ref, queries, *args)
        wall = time.perf_counter() - t0
        print('map_queries default path, %-12s %d queries of %d against %d: wall %.4f s   (%d alignments)'
              % (label, len(queries), sh['qlen'], len(ref), wall, sum(r['alignment'] is not None for recs in got for r in recs)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=10000)
    ap.add_argument('--runs', type=int, default=25)
    ap.add_argument('--map-repeats', type=int, default=3)
    ap.add_argument('--no-map', action='store_true')
    ap.add_argument('--default-only', action='store_true')
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(HERE)))
    ap.add_argument('--label', default='this commit')
    args = ap.parse_args()
    _import_from(os.path.abspath(args.root))
    if args.default_only:
        return default_only(args.label, args.map_repeats)
    assert args.runs >= 20, 'the medians are taken over at least 20 runs'
    config2(args.pairs, args.runs)
    if not args.no_map:
        mapping_batch(args.runs)
        mapping_walls(args.map_repeats)


if __name__ == '__main__':
    main()
