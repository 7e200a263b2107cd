"""The iterated consensus on the device (K20, pw_rounds.hip): the column polish beside the per-read polish, and the rounds.

    python tests/micro/consensus_rounds_bench.py [--reads N] [--read-len N] [--reps R] [--rounds K] [--eval-letters N] [--gate]

The read set, the overlaps and the graph of tests/micro/consensus_bench.py.  Two measurements.

Polish timing.  One layout, one pileup filled as OverlapGraph.consensus fills it; then, in this process and on that pileup,
pw_pileup_polish (K16's kernels, one wavefront per contig) and pw_pileup_polish_columns (one lane per column) ALTERNATE:
2 untimed calls each, then R timed ones each, a host clock around the synchronous calls.  Reported: median, min and max of
either, the ratio of the medians and the run-to-run spread (max - min) of either beside it.  After every pair of calls the
letters, offsets and statistics of the two are compared byte for byte; a difference ends the run.  --gate makes the run fail
unless the column polish's median plus both spreads lies below the per-read polish's median.

Rounds.  OverlapGraph.consensus(rounds=k) for k = 1 .. K after one untimed run: the per-round host times around synchronised
work (layout or relayout, align, polish), tasks, aligned, the polish records summed, and the error total of the contigs that
k rounds return (the measure of tests/micro/consensus_bench.py, over the first --eval-letters letters).  No time is asserted
here."""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cigar_bench as CB                                  # noqa: E402  (the import helper)
import consensus_bench as KB                              # noqa: E402  (the error measure)

COMP = KB.COMP


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=5000)
    ap.add_argument('--read-len', type=int, default=5000)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--eval-letters', type=int, default=200000)
    ap.add_argument('--gate', action='store_true')
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(HERE))
    CB._import_from(root)
    sys.path.insert(0, root)
    from biseqt_amd import synth
    from biseqt_amd.batch import POLISH_STATS_DTYPE, DeviceArena, Pileup, pack_reads
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
    found = overlap_all_pairs(reads, KB.K, A, .2, .9, strands='both', complement=COMP)
    keys = [k for k, band in found.items() if band is not None and band['p'] >= .8]
    print('%d reads of about %d letters from both strands (genome %d, 25x), %d candidate pairs, %d with p >= .8'
          % (R, n, G, len(found), len(keys)), flush=True)
    arena, offs, _ = pack_reads(reads)
    ok = True
    with OverlapGraph(lens) as Gr, DeviceArena(arena) as dev:
        overlap_alignments(reads, [(k[0], k[1]) for k in keys], [found[k] for k in keys], A, want_transcripts=False,
                           strands=[k[2] for k in keys], complement=COMP, graph=Gr)
        Gr.build()
        draft = Gr.contigs((dev, offs), COMP)
        unitigs, members = Gr.unitigs()
        # ---- the two polishes on one pileup ----
        cstart, tasks, carena = Gr.consensus_layout((dev, offs), COMP)
        n_cols = int(cstart[-1])
        coffs = np.ascontiguousarray(cstart[:-1], np.int64)
        clens = np.ascontiguousarray(unitigs['length'], np.int32)
        lib = Gr.lib
        with Pileup(n_cols, 4, ins_slots=2) as pile:
            aligned = Gr._pile_tasks(pile, tasks, carena, 4, 1, 2 * 10 ** 10, {})
            print('one pileup of %d columns over %d contigs (%d tasks, %d aligned); min_depth 3, two insertion slots'
                  % (n_cols, len(clens), len(tasks), aligned), flush=True)

            def call(name):
                t0 = time.perf_counter()
                rc = getattr(lib, name)(pile.handle, carena.ptr, coffs.ctypes.data, clens.ctypes.data, len(coffs), 3, None)
                ms = 1e3 * (time.perf_counter() - t0)
                assert rc == 0, name
                total = int(lib.pw_pileup_polished_total(pile.handle))
                letters, poffs = np.zeros(total, np.uint8), np.zeros(len(coffs) + 1, np.int64)
                st = np.zeros(len(coffs), POLISH_STATS_DTYPE)
                assert lib.pw_pileup_polished_letters(pile.handle, letters.ctypes.data) == 0
                assert lib.pw_pileup_polished_offsets(pile.handle, poffs.ctypes.data) == 0
                assert lib.pw_pileup_polished_stats(pile.handle, st.ctypes.data) == 0
                return ms, (letters.tobytes(), poffs.tobytes(), st.tobytes())

            t_read, t_col = [], []
            for r in range(2 + args.reps):
                ms_r, out_r = call('pw_pileup_polish')
                ms_c, out_c = call('pw_pileup_polish_columns')
                if out_r != out_c:
                    print('THE TWO POLISHES DIFFER in repetition %d' % r)
                    sys.exit(1)
                if r >= 2:
                    t_read.append(ms_r); t_col.append(ms_c)
            colmap = pile.colmap()
            assert int(colmap[-1]) == len(out_c[0])
        CB.stats('pw_pileup_polish (per read; host clock around the call)', t_read, '   max %.4f ms' % max(t_read))
        CB.stats('pw_pileup_polish_columns (per column; likewise)', t_col, '   max %.4f ms' % max(t_col))
        m_r, m_c = float(np.median(t_read)), float(np.median(t_col))
        s_r, s_c = max(t_read) - min(t_read), max(t_col) - min(t_col)
        print('outputs byte-equal in all %d repetitions (%d letters).  per read / per column: %.2f   (run-to-run spread, max - min: %.4f ms and %.4f ms)'
              % (2 + args.reps, len(out_c[0]), m_r / m_c, s_r, s_c), flush=True)
        if args.gate:
            ok = m_c + s_r + s_c < m_r
            print('gate (column median + both spreads < per-read median): %s' % ('holds' if ok else 'FAILS'), flush=True)
        # ---- the rounds ----
        Gr.consensus((dev, offs), 4, COMP, rounds=2)                            # untimed
        results = []
        for k in range(1, args.rounds + 1):
            stats = {}
            contigs, records = Gr.consensus((dev, offs), 4, COMP, stats=stats, rounds=k)
            results.append((k, contigs, stats))
            if len(stats['rounds']) < k:
                break                                                           # the fixed point: more rounds return the same
        for q, r in enumerate(results[-1][2]['rounds']):
            print('round %d: layout %.4f ms, align %.4f ms, polish %.4f ms; tasks %d, aligned %d; kept %d, substituted %d, deleted %d, inserted %d'
                  % ((q + 1, r['layout_ms'], r['align_ms'], r['polish_ms'], r['tasks'], r['aligned'])
                     + tuple(int(r['records'][f].sum()) for f in ('kept', 'substituted', 'deleted', 'inserted'))), flush=True)
    t0 = time.perf_counter()
    e0, n0 = KB.error_total(draft, draft, unitigs, members, starts, minus, n, g, args.eval_letters)
    print('error total over pieces of %d letters, the first %d letters: draft %d over %d letters (%.3f %%)'
          % (KB.PIECE, args.eval_letters, e0, n0, 100. * e0 / max(n0, 1)), flush=True)
    for k, contigs, stats in results:
        e, m = KB.error_total(contigs, draft, unitigs, members, starts, minus, n, g, args.eval_letters)
        print('  rounds=%d (%d ran): contigs of %d letters; errors %d over %d letters (%.4f %%)'
              % (k, len(stats['rounds']), sum(len(c) for c in contigs), e, m, 100. * e / max(m, 1)), flush=True)
    print('[host, %.0f s]' % (time.perf_counter() - t0), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
