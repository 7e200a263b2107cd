"""The consensus stage on the device (pw_consensus.hip, OverlapGraph.consensus) beside the alignment stage that feeds the graph.

    python tests/micro/consensus_bench.py [--reads N] [--read-len N] [--runs R] [--eval-letters N]

The read set of tests/micro/graph_bench.py (25x coverage of a random genome, reads from both strands, .05 / .025 / .025
errors as in tests/micro/polish_bench.py).  The overlaps come from overlap_all_pairs (k = 16, both strands); the pairs with
p >= .8 are aligned in B_OVERLAP batches (1 / -3 / -5 / -2) by overlap_alignments(want_transcripts=False, graph=G), whose
host wall time is the alignment stage of the layout.  After build and contigs, OverlapGraph.consensus runs R times after one
untimed run and reports its own three host times around synchronised work -- layout (placements, tasks, arena), align (the
read-against-contig batches and their adds) and polish -- and pw_graph_consensus_layout alone between two HIP events.
Reported beside the times: placed reads, tasks, the bytes the graph holds on the device with the consensus arrays, and the
contigs' error totals before and after: every contig is cut into pieces of 2000 letters, each piece is compared with the
stretch of the genome where its member reads come from (600 letters of margin on either side, the genome's flanks free),
and the unit-cost edit distances are summed -- over the first --eval-letters letters of the contigs (default: all).  No time
is asserted."""
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
PIECE, MARGIN = 2000, 600


def infix_distance(piece, window):
    a, b = np.asarray(piece, np.int64), np.asarray(window, np.int64)
    idx = np.arange(len(b) + 1)
    prev = np.zeros(len(b) + 1, np.int64)
    for x in a:
        t = np.empty(len(b) + 1, np.int64)
        t[0] = prev[0] + 1
        t[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (b != x))
        prev = np.minimum.accumulate(t - idx) + idx
    return int(prev.min())


def error_total(contigs, drafts, unitigs, members, starts, minus, span, genome, budget):
    """Sum of the pieces' distances; ``drafts`` gives the coordinates the member offsets are in."""
    total = letters = 0
    for u, c in enumerate(contigs):
        mem = members[int(unitigs['first_member'][u]):int(unitigs['first_member'][u]) + int(unitigs['n_members'][u])]
        scale = len(drafts[u]) / max(len(c), 1)
        for p in range(0, len(c), PIECE):
            if letters >= budget:
                return total, letters
            piece = c[p:p + PIECE]
            at = p * scale
            m = mem[max(int(np.searchsorted(mem['offset'], at, 'right')) - 1, 0)]
            r, o = int(m['vertex']) >> 1, int(m['vertex']) & 1
            fwd = bool(minus[r]) == bool(o)
            d = int(at - int(m['offset']))
            if fwd:
                g = int(starts[r]) + d
                window = genome[max(g - MARGIN, 0):g + len(piece) + MARGIN]
            else:
                g = int(starts[r]) + span - d
                window = COMP[genome[max(g - len(piece) - MARGIN, 0):g + MARGIN][::-1]]
            total += infix_distance(piece, window)
            letters += len(piece)
    return total, letters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=5000)
    ap.add_argument('--read-len', type=int, default=5000)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--eval-letters', type=int, default=1 << 40)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(HERE))
    CB._import_from(root)
    sys.path.insert(0, root)
    from biseqt_amd import synth
    from biseqt_amd.batch import DeviceArena, pack_reads
    from biseqt_amd.graph import OverlapGraph
    from biseqt_amd.overlap import overlap_alignments, overlap_all_pairs
    from biseqt_amd.sequence import Alphabet
    A = Alphabet('ACGT')
    rng = synth.rng_for(4)
    R, n = args.reads, args.read_len
    G = R * n // 25
    g = synth.rand_seqs(rng, 1, G)[0]
    starts = rng.integers(0, G - n, R)
    minus = rng.random(R) < .5
    reads = [synth.mutate(rng, COMP[g[s:s + n][::-1]] if neg else g[s:s + n], .05, .025, .025) for s, neg in zip(starts.tolist(), minus.tolist())]
    lens = [len(r) for r in reads]
    found = overlap_all_pairs(reads, K, A, .2, .9, strands='both', complement=COMP)
    keys = [k for k, band in found.items() if band is not None and band['p'] >= .8]
    print('%d reads of about %d letters from both strands (genome %d, 25x), %d candidate pairs, %d with p >= .8'
          % (R, n, G, len(found), len(keys)), flush=True)
    ev = CB.Events(CB.hip_runtime(), 2)
    arena, offs, _ = pack_reads(reads)
    with OverlapGraph(lens) as Gr, DeviceArena(arena) as dev:
        t0 = time.perf_counter()
        alns = overlap_alignments(reads, [(k[0], k[1]) for k in keys], [found[k] for k in keys], A, want_transcripts=False,
                                  strands=[k[2] for k in keys], complement=COMP, graph=Gr)
        align_ms = 1e3 * (time.perf_counter() - t0)
        print('alignment stage of the layout (overlap_alignments, no transcripts, records appended to the graph): host wall %.1f ms, %d of %d pairs aligned'
              % (align_ms, sum(a is not None for a in alns), len(keys)), flush=True)
        Gr.build()
        before_bytes = Gr.device_bytes
        draft = Gr.contigs((dev, offs), COMP)
        unitigs, members = Gr.unitigs()
        tl, ta, tp, tk = [], [], [], []
        for r in range(1 + args.runs):
            stats = {}
            contigs, records = Gr.consensus((dev, offs), 4, COMP, stats=stats)
            if r >= 1:
                tl.append(stats['layout_ms']); ta.append(stats['align_ms']); tp.append(stats['polish_ms'])
        for r in range(1 + args.runs):
            ev.record(0)
            Gr.lib.pw_graph_consensus_layout(Gr.handle, dev.ptr, offs.ctypes.data, COMP.ctypes.data, 4, 50, .1, None)
            ev.record(1)
            if r >= 1:
                tk.append(ev.ms(0, 1))
        CB.stats('consensus: layout (host wall)', tl, '   max %.4f ms' % max(tl))
        CB.stats('  pw_graph_consensus_layout (events around the call)', tk, '   max %.4f ms' % max(tk))
        CB.stats('consensus: align (host wall, batches and adds)', ta, '   max %.4f ms' % max(ta))
        CB.stats('consensus: polish (host wall)', tp, '   max %.4f ms' % max(tp))
        print('consensus stage / alignment stage of the layout: %.3f' % ((np.median(tl) + np.median(ta) + np.median(tp)) / align_ms))
        print('placed %d, unplaced %d, tasks %d, aligned %d; contigs %d, letters %d -> %d'
              % (stats['placed'], stats['unplaced'], stats['tasks'], stats['aligned'], len(contigs), sum(len(c) for c in draft),
                 sum(len(c) for c in contigs)))
        print('polish records summed: kept %d, substituted %d, deleted %d, inserted %d'
              % tuple(int(records[f].sum()) for f in ('kept', 'substituted', 'deleted', 'inserted')))
        print('the graph holds %.1f MB on the device after the build, %.1f MB with the consensus arrays'
              % (before_bytes / 1e6, Gr.device_bytes / 1e6), flush=True)
    ev.close()
    t0 = time.perf_counter()
    e0, n0 = error_total(draft, draft, unitigs, members, starts, minus, n, g, args.eval_letters)
    e1, n1 = error_total(contigs, draft, unitigs, members, starts, minus, n, g, args.eval_letters)
    print('error total over pieces of %d letters: draft %d over %d letters (%.3f %%), polished %d over %d letters (%.4f %%)   [host, %.0f s]'
          % (PIECE, e0, n0, 100. * e0 / max(n0, 1), e1, n1, 100. * e1 / max(n1, 1), time.perf_counter() - t0), flush=True)


if __name__ == '__main__':
    main()
