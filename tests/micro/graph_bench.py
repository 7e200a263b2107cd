"""The overlap graph on the device (pw_graph.hip) beside the alignment stage that feeds it and the CPU oracle.

    python tests/micro/graph_bench.py [--reads N] [--read-len N] [--runs R] [--oracle-reads N]

A read set shaped like config 4 (tests/micro/overlap_all_bench.py: 25x coverage of a random genome, .05 / .025 / .025 errors),
reads from both strands.  The overlaps come from overlap_all_pairs (k = 16, both strands); the pairs with p >= .8 are aligned
in B_OVERLAP batches (1 / -3 / -5 / -2) by overlap_alignments(want_transcripts=False, graph=G), whose host wall time -- the
work is synchronised batch by batch -- is the alignment stage.  Then, in this process, R runs after two untimed ones, each
between two HIP events on the default stream around the synchronous call: pw_graph_build (default parameters) with the time
of its reduction kernel, and pw_graph_contigs on letters that are on the device already.  tests/graph_ref.py is timed on the
host on the records among the first --oracle-reads reads and scaled by the record count (labelled so).  Reported beside the
times: records by class, arcs, kept arcs, the row-length histogram of the arc table, unitigs, the N50 of the contig lengths
and the bytes the graph holds on the device.  No time is asserted."""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cigar_bench as CB                                  # noqa: E402  (the event helpers)

K = 16
COMP = np.array([3, 2, 1, 0], np.uint8)


def n50(lengths):
    lengths = sorted((int(x) for x in lengths), reverse=True)
    half, acc = sum(lengths) / 2., 0
    for x in lengths:
        acc += x
        if acc >= half:
            return x
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=5000)
    ap.add_argument('--read-len', type=int, default=5000)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--oracle-reads', type=int, default=500)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(HERE))
    CB._import_from(root)
    sys.path.insert(0, root)
    from biseqt_amd import synth
    from biseqt_amd.batch import DeviceArena, pack_reads
    from biseqt_amd.graph import ARC_REMOVED, CLASS_NAMES, OverlapGraph
    from biseqt_amd.overlap import overlap_alignments, overlap_all_pairs
    from biseqt_amd.sequence import Alphabet
    from tests import graph_ref
    A = Alphabet('ACGT')
    rng = synth.rng_for(4)
    R, n = args.reads, args.read_len
    G = R * n // 25
    g = synth.rand_seqs(rng, 1, G)[0]
    starts = rng.integers(0, G - n, R)
    minus = rng.random(R) < .5
    reads = [synth.mutate(rng, COMP[g[s:s + n][::-1]] if neg else g[s:s + n], .05, .025, .025) for s, neg in zip(starts.tolist(), minus.tolist())]
    lens = [len(r) for r in reads]
    t0 = time.perf_counter()
    ostats = {}
    found = overlap_all_pairs(reads, K, A, .2, .9, strands='both', complement=COMP, stats=ostats)
    t1 = time.perf_counter()
    keys = [k for k, band in found.items() if band is not None and band['p'] >= .8]
    print('%d reads of about %d letters from both strands (genome %d, 25x), %d candidate pairs, %d with p >= .8'
          % (R, n, G, len(found), len(keys)), flush=True)
    print('overlap_all_pairs: host wall %.1f ms (device %.1f ms)' % (1e3 * (t1 - t0), ostats['device_ms']), flush=True)
    ev = CB.Events(CB.hip_runtime(), 2)
    arena, offs, _ = pack_reads(reads)
    with OverlapGraph(lens) as Gr, DeviceArena(arena) as dev:
        t0 = time.perf_counter()
        alns = overlap_alignments(reads, [(k[0], k[1]) for k in keys], [found[k] for k in keys], A, want_transcripts=False,
                                  strands=[k[2] for k in keys], complement=COMP, graph=Gr)
        align_ms = 1e3 * (time.perf_counter() - t0)
        print('alignment stage (overlap_alignments, no transcripts, records appended to the graph): host wall %.1f ms, %d of %d pairs aligned'
              % (align_ms, sum(a is not None for a in alns), len(keys)), flush=True)
        tb, tr, tc, wall = [], [], [], []
        for r in range(2 + args.runs):
            w0 = time.perf_counter()
            ev.record(0); Gr.build(); ev.record(1)
            ms = ev.ms(0, 1)
            w1 = time.perf_counter()
            if r >= 2:
                tb.append(ms); tr.append(Gr.reduce_ms); wall.append(1e3 * (w1 - w0))
        for r in range(2 + args.runs):
            ev.record(0); Gr.lib.pw_graph_contigs(Gr.handle, dev.ptr, offs.ctypes.data, COMP.ctypes.data, 4, None); ev.record(1)
            ms = ev.ms(0, 1)
            if r >= 2:
                tc.append(ms)
        CB.stats('pw_graph_build (events around the call)', tb, '   max %.4f ms' % max(tb))
        CB.stats('  of which k_graph_reduce', tr, '   max %.4f ms' % max(tr))
        CB.stats('pw_graph_build (host wall)', wall, '   max %.4f ms' % max(wall))
        CB.stats('pw_graph_contigs (events around the call)', tc, '   max %.4f ms' % max(tc))
        print('graph stage / alignment stage: build %.4f, build + contigs %.4f'
              % (np.median(tb) / align_ms, (np.median(tb) + np.median(tc)) / align_ms), flush=True)
        recs = Gr.overlaps()
        arcs, rows = Gr.arcs()
        unitigs, members = Gr.unitigs()
        contained = Gr.contained()
        print('records %d: %s' % (len(recs), ', '.join('%s %d' % (CLASS_NAMES[c], int((recs['cls'] == c).sum())) for c in range(7))))
        print('contained reads %d of %d; arcs %d, kept %d; unitigs %d with %d members; contig letters %d, N50 %d, longest %d'
              % (int(contained.sum()), R, len(arcs), int((arcs['flags'] & ARC_REMOVED == 0).sum()), len(unitigs), len(members),
                 int(unitigs['length'].sum()), n50(unitigs['length']), int(unitigs['length'].max()) if len(unitigs) else 0))
        deg = np.diff(rows)
        edges = [0, 1, 2, 4, 8, 16, 32, 64, 128, 256, 1 << 30]
        print('row lengths of the arc table (arcs leaving a vertex): ' +
              ', '.join('[%d, %s) %d' % (lo, hi if hi < 1 << 30 else 'inf', int(((deg >= lo) & (deg < hi)).sum())) for lo, hi in zip(edges, edges[1:]))
              + '; longest %d' % (int(deg.max()) if len(deg) else 0))
        print('the graph holds %.1f MB on the device' % (Gr.device_bytes / 1e6), flush=True)
    ev.close()
    m = min(args.oracle_reads, R)
    fields = ('a', 'b', 'strand', 'a_beg', 'a_end', 'b_beg', 'b_end', 'n_match', 'n_ops')
    sub = [tuple(int(r[f]) for f in fields) for r in recs[(recs['a'] < m) & (recs['b'] < m)]]
    t0 = time.perf_counter()
    graph_ref.build(lens[:m], sub)
    ref_ms = 1e3 * (time.perf_counter() - t0)
    print('tests/graph_ref.py on the host: %.1f ms for the %d records among the first %d reads; SCALED by the record count to all %d records: %.0f ms'
          % (ref_ms, len(sub), m, len(recs), ref_ms * len(recs) / max(len(sub), 1)), flush=True)


if __name__ == '__main__':
    main()
