"""Tip removal and bubble popping (pw_clean.hip, K19) on the read set of tests/micro/graph_bench.py, and on the same read set
with 1 % of the reads given a junk tail.

    python tests/micro/graph_clean_bench.py [--reads N] [--read-len N] [--runs R] [--save-records DIR] [--records DIR]

The stock case is graph_bench.py's: 25x coverage of a random genome by reads from both strands with .05 / .025 / .025 errors,
overlaps from overlap_all_pairs (k = 16), the pairs with p >= .8 aligned into the graph by overlap_alignments.  The second case
replaces the last third of every hundredth read with random letters before the overlaps are looked for.  On either graph, R
runs after two untimed ones, each between two HIP events on the default stream around the synchronous call: pw_graph_build,
and pw_graph_build_clean with max_tip_reads = 4, max_bubble_reads = 8 at one round and at two.  Beside the times: unitigs,
N50 and longest contig, the reads dropped as tips and as bubbles, kept arcs, the vertices that still branch (two kept arcs or
more leaving them, and how many of them are transitive arcs that the reduction left) and the bytes the graph holds on the
device.  The same three builds are then repeated with min_identity = .7, which classes an overlap that runs through a junk
tail as WEAK.  --save-records writes lens_<case>.npy / records_<case>.npy;
--records DIR times the builds on such files alone (no overlap stage: an A/B of two builds on one set of records).  No time
is asserted."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cigar_bench as CB                                  # noqa: E402  (the event helpers)
from graph_bench import COMP, K, n50                      # noqa: E402

SETTINGS = (('pw_graph_build (cleaning off)', {}),
            ('pw_graph_build_clean tips 4, bubbles 8, 1 round', dict(max_tip_reads=4, max_bubble_reads=8, clean_rounds=1)),
            ('pw_graph_build_clean tips 4, bubbles 8, 2 rounds', dict(max_tip_reads=4, max_bubble_reads=8, clean_rounds=2)))


def branches(kept):
    """What the vertices with two kept arcs or more are: for every pair of kept arcs v -> w1, v -> w2 with a kept arc w1 -> w2
    the detour's excess len(v -> w1) + len(w1 -> w2) - len(v -> w2) -- a transitive arc that the reduction left because the
    excess is above fuzz.  Returns ``(branching vertices, those with such a pair, the excesses)``."""
    rows = {}
    for v, w, ln in zip(kept['v'].tolist(), kept['w'].tolist(), kept['len'].tolist()):
        rows.setdefault(v, []).append((w, ln))
    forks = [v for v, row in rows.items() if len(row) >= 2]
    explained, excess = 0, []
    for v in forks:
        found = [l1 + l12 - l2 for w1, l1 in rows[v] for w2, l2 in rows[v] if w1 != w2 for x, l12 in rows.get(w1, []) if x == w2]
        explained += bool(found)
        excess += found
    return len(forks), explained, sorted(excess)


def time_builds(Gr, ev, runs, settings=SETTINGS, **params):
    from biseqt_amd.graph import ARC_REMOVED
    for name, kw in settings:
        kw = dict(kw, **params)
        t = []
        for r in range(2 + runs):
            ev.record(0); Gr.build(**kw); ev.record(1)
            ms = ev.ms(0, 1)
            if r >= 2:
                t.append(ms)
        CB.stats(name, t, '   max %.4f ms   all %s' % (max(t), ' '.join('%.4f' % x for x in t)))
        arcs, rows = Gr.arcs()
        unitigs, members = Gr.unitigs()
        kept = arcs[arcs['flags'] & ARC_REMOVED == 0]
        out = np.bincount(kept['v'], minlength=len(rows) - 1)
        gone = Gr.dropped() if hasattr(Gr, 'dropped') else np.zeros(0, np.uint8)
        print('    unitigs %d with %d members, N50 %d, longest %d; dropped: %d tips, %d bubbles; kept arcs %d; branching vertices %d; %.1f MB on the device'
              % (len(unitigs), len(members), n50(unitigs['length']), int(unitigs['length'].max()) if len(unitigs) else 0,
                 int((gone == 1).sum()), int((gone == 2).sum()), len(kept), int((out >= 2).sum()), Gr.device_bytes / 1e6), flush=True)
        n_forks, explained, excess = branches(kept)
        print('    of the %d branching vertices %d have a kept arc between two of their targets (a transitive arc left by the reduction); '
              'len(v->w1) + len(w1->w2) - len(v->w2): %s' % (n_forks, explained, ' '.join(str(x) for x in excess[:40])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=5000)
    ap.add_argument('--read-len', type=int, default=5000)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--save-records', default=None)
    ap.add_argument('--records', default=None)
    ap.add_argument('--plain-only', action='store_true', help='with --records: time pw_graph_build alone (a build without the cleaning surface)')
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(HERE))
    CB._import_from(root)
    sys.path.insert(0, root)
    from biseqt_amd import synth
    from biseqt_amd.graph import OverlapGraph
    ev = CB.Events(CB.hip_runtime(), 2)
    if args.records:
        for case in ('stock', 'junk'):
            lens, recs = np.load(os.path.join(args.records, 'lens_%s.npy' % case)), np.load(os.path.join(args.records, 'records_%s.npy' % case))
            print('%s: %d reads, %d records from %s' % (case, len(lens), len(recs), args.records), flush=True)
            with OverlapGraph(lens) as Gr:
                Gr.add(recs)
                time_builds(Gr, ev, args.runs, SETTINGS[:1] if args.plain_only else SETTINGS)
        ev.close()
        return
    from biseqt_amd.overlap import overlap_alignments, overlap_all_pairs
    from biseqt_amd.sequence import Alphabet
    A = Alphabet('ACGT')
    rng = synth.rng_for(4)
    R, n = args.reads, args.read_len
    G = R * n // 25
    g = synth.rand_seqs(rng, 1, G)[0]
    starts = rng.integers(0, G - n, R)
    minus = rng.random(R) < .5
    stock = [synth.mutate(rng, COMP[g[s:s + n][::-1]] if neg else g[s:s + n], .05, .025, .025) for s, neg in zip(starts.tolist(), minus.tolist())]
    junk = [r.copy() for r in stock]
    for q in range(0, R, 100):                              # 1 %: every hundredth read ends in random letters
        tail = len(junk[q]) // 3
        junk[q][len(junk[q]) - tail:] = rng.integers(0, 4, tail, dtype=np.uint8)
    for case, reads in (('stock', stock), ('junk', junk)):
        lens = [len(r) for r in reads]
        found = overlap_all_pairs(reads, K, A, .2, .9, strands='both', complement=COMP)
        keys = [k for k, band in found.items() if band is not None and band['p'] >= .8]
        print('%s: %d reads of about %d letters from both strands (genome %d, 25x)%s, %d candidate pairs, %d with p >= .8'
              % (case, R, n, G, '' if case == 'stock' else ', %d of them with a junk tail' % len(range(0, R, 100)), len(found), len(keys)), flush=True)
        with OverlapGraph(lens) as Gr:
            overlap_alignments(reads, [(k[0], k[1]) for k in keys], [found[k] for k in keys], A, want_transcripts=False,
                               strands=[k[2] for k in keys], complement=COMP, graph=Gr)
            time_builds(Gr, ev, args.runs)
            planted = np.zeros(R, bool)
            planted[::100] = case == 'junk'

            def fate():
                gone, inside = Gr.dropped(), Gr.contained()
                print('    of the %d junk-tailed reads %d are dropped (%d contained); %d other reads are dropped'
                      % (int(planted.sum()), int((gone[planted] > 0).sum()), int(inside[planted].sum()), int((gone[~planted] > 0).sum())), flush=True)
            fate()
            # Two reads with these error rates agree in about .82 of the alignment's columns, an overlap that runs through a junk
            # tail in far fewer: with an identity bound between the two the junk overlaps are WEAK, not dovetails.
            recs = Gr.overlaps()
            ident = recs['n_match'][recs['n_ops'] > 0] / recs['n_ops'][recs['n_ops'] > 0]
            print('%s, min_identity = .7 (identity n_match / n_ops of the records: 1 %% %.3f, 10 %% %.3f, median %.3f):'
                  % (case, np.percentile(ident, 1), np.percentile(ident, 10), np.median(ident)), flush=True)
            time_builds(Gr, ev, args.runs, min_identity=.7)
            fate()
            if args.save_records:
                os.makedirs(args.save_records, exist_ok=True)
                np.save(os.path.join(args.save_records, 'lens_%s.npy' % case), np.array(lens, np.int32))
                np.save(os.path.join(args.save_records, 'records_%s.npy' % case), Gr.overlaps())
    ev.close()


if __name__ == '__main__':
    main()
