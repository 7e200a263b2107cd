"""Alignment summaries on the device (pw_txsum.hip) beside what they stand next to.

    python tests/micro/tx_summary_bench.py [--pairs N] [--runs R] [--no-map]

Part 1, BASELINE config 2 (10 000 pairs of 2 kb, band radius 200, B_LOCAL, 1 / -3 / -5 / -2), one solved batch, R runs
after three untimed ones: device milliseconds of pw_batch_summarize and of pw_batch_pack_transcripts -- its two kernels
read the same op bytes and also write them -- each between two HIP events recorded around the call on the default stream,
and pw_batch_trace_ms of the traceback in front of them.  Medians and minima.

Part 2, the read-mapping shape of tests/micro/blot_many_bench.py (10 000 queries of 250 letters against 100 kb): host wall
seconds of pipeline.map_queries with alignments=True (transcripts downloaded, decoded, counted as strings) and with
alignments=False (records and summaries only), after one untimed call of each on 8 queries; the clocks end with the
results on the host."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from biseqt_amd import _pwlib as W            # noqa: E402
from biseqt_amd import synth                  # noqa: E402
from biseqt_amd.batch import BatchAligner     # noqa: E402


def hip_runtime():
    """The HIP runtime pwlib.so is bound to (the one mapped into this process), for the events."""
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
    print('%-44s median %8.4f ms   min %8.4f ms   (%d runs)%s' % (name, float(np.median(v)), min(v), len(v), extra), flush=True)


def kernels(n_pairs, runs):
    hip = hip_runtime()
    origins, mutants = synth.pair_batch(2, n_pairs, 2000)
    with BatchAligner(list(zip(origins, mutants)), alnmode=1, alntype=1, alphabet_len=4, diag_range=(-200, 200), match_score=1,
                      mismatch_score=-3, go_score=-5, ge_score=-2, flags=W.PW_FLAG_PROFILE) as b:
        ev = Events(hip, 4)
        b.solve()
        t_sum, t_pack, t_trace = [], [], []
        for r in range(3 + runs):
            b.traceback()
            ev.record(0); b.summarize(); ev.record(1)
            ev.record(2); b.pack_transcripts(); ev.record(3)
            b.sync()
            if r >= 3:
                t_sum.append(ev.ms(0, 1)); t_pack.append(ev.ms(2, 3)); t_trace.append(b.trace_ms())
        res, sums = b.results(), b.summaries()
        ops = int(np.maximum(res['tx_len'], 0).sum())
        assert int(sums['n_match'].sum() + sums['n_subst'].sum() + sums['n_ins'].sum() + sums['n_del'].sum()) == ops
        print('config 2: %d pairs of 2 kb, band radius 200, B_LOCAL; %s; %d ops in %d transcripts (%.0f per transcript)' %
              (n_pairs, b.kernel_name, ops, int((sums['flags'] == 1).sum()), ops / max(1, int((sums['flags'] == 1).sum()))), flush=True)
        stats('pw_batch_summarize (k_tx_summary)', t_sum, '   %.1f GB/s of ops read' % (ops / np.median(t_sum) / 1e6))
        stats('pw_batch_pack_transcripts (offsets + pack)', t_pack, '   %.1f GB/s of ops read' % (ops / np.median(t_pack) / 1e6))
        stats('pw_batch_trace_ms (walk + fix-up)', t_trace)
        print('summarize / pack_transcripts (medians): %.2f' % (np.median(t_sum) / np.median(t_pack)), flush=True)
        ev.close()


def mapping(repeats):
    import blot_many_bench as M
    from biseqt_amd.pipeline import map_queries
    sh = M.SHAPES['map']
    ref, queries = M.make('map', sh['queries'])
    args = (sh['K_min'], M.P_MIN, sh['wordlen'], M.G_MAX, M.SENS)
    out = {}
    for alignments in (True, False):
        map_queries(ref, queries[:8], *args, alignments=alignments)
        walls = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            got = map_queries(ref, queries, *args, alignments=alignments)
            walls.append(time.perf_counter() - t0)
        out[alignments] = (walls, got)
        n_aln = sum(r['score'] is not None for recs in got for r in recs)
        print('map_queries, %d queries of %d against %d, alignments=%-5s  wall median %.4f s   min %.4f s   (%d calls; %d alignments)'
              % (len(queries), sh['qlen'], len(ref), alignments, float(np.median(walls)), min(walls), repeats, n_aln), flush=True)
    full, lean = out[True][1], out[False][1]
    assert all(f['p_aln'] == l['p_aln'] and f['len_aln'] == l['len_aln'] and f['score'] == l['score']
               for fr, lr in zip(full, lean) for f, l in zip(fr, lr))
    print('alignments=False / alignments=True (medians): %.2f' % (np.median(out[False][0]) / np.median(out[True][0])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=10000)
    ap.add_argument('--runs', type=int, default=25)
    ap.add_argument('--map-repeats', type=int, default=5)
    ap.add_argument('--no-map', action='store_true')
    args = ap.parse_args()
    assert args.runs >= 20, 'the medians are taken over at least 20 runs'
    kernels(args.pairs, args.runs)
    if not args.no_map:
        mapping(args.map_repeats)


if __name__ == '__main__':
    main()
