"""Read correction on the device (pw_polish.hip) beside the one-sided pileup add it extends.

    python tests/micro/polish_bench.py [--reads N] [--read-len N] [--runs R] [--eval N]

A read set shaped like config 4 (tests/micro/overlap_all_bench.py: 25x coverage of a random genome, .05 / .025 / .025 errors),
small enough for a minute, reads from both strands.  The overlaps come from overlap_all_pairs (k = 16, both strands), the
pairs with p >= .8 are aligned in B_OVERLAP batches (1 / -3 / -5 / -2).  On every batch, in this process, R runs after three
untimed ones, each between two HIP events on the default stream with the pileups cleared outside the events: the parent's
pw_batch_pileup_add (origin side, no plane) -- the yardstick --, pw_batch_pileup_add_sides for the origin side alone into a
pileup with two insertion slots, and for both sides (minus pairs reversed).  Then the self vote (events), the polish (host
wall: the call is synchronous), the whole correct_reads (host wall), and the total edit distance to the truth of the first
--eval reads before and after.  No time is asserted."""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cigar_bench as CB                                  # noqa: E402  (the event helpers)

L, K = 4, 16
COMP = np.array([3, 2, 1, 0], np.uint8)


def edit_distance(a, b):
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    idx = np.arange(len(b) + 1)
    prev = idx.copy()
    for x in a:
        t = np.empty(len(b) + 1, np.int64)
        t[0] = prev[0] + 1
        t[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (b != x))
        prev = np.minimum.accumulate(t - idx) + idx
    return int(prev[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=300)
    ap.add_argument('--read-len', type=int, default=2000)
    ap.add_argument('--runs', type=int, default=25)
    ap.add_argument('--eval', type=int, default=60)
    args = ap.parse_args()
    CB._import_from(os.path.dirname(os.path.dirname(HERE)))
    from biseqt_amd import synth
    from biseqt_amd.batch import DeviceArena, Pileup, pack_reads
    from biseqt_amd.overlap import aligned_batches, correct_reads, overlap_all_pairs
    from biseqt_amd.sequence import Alphabet
    A = Alphabet('ACGT')
    rng = synth.rng_for(4)
    R, n = args.reads, args.read_len
    G = R * n // 25
    g = synth.rand_seqs(rng, 1, G)[0]
    starts = rng.integers(0, G - n, R)
    minus = rng.random(R) < .5
    truth = [COMP[g[s:s + n][::-1]] if neg else g[s:s + n] for s, neg in zip(starts.tolist(), minus.tolist())]
    reads = [synth.mutate(rng, t, .05, .025, .025) for t in truth]
    found = overlap_all_pairs(reads, K, A, .2, .9, strands='both', complement=COMP)
    keys = [k for k, band in found.items() if band is not None and band['p'] >= .8]
    arena, offs, lens = pack_reads(reads)
    pidx = np.array([(a, b) for a, b, _ in keys], np.int64)
    rev = np.array([st == '-' for _, _, st in keys], np.uint8)
    dr = np.array([(max(found[k]['d_band'][0], -int(lens[k[1]])), min(found[k]['d_band'][1], int(lens[k[0]]))) for k in keys], np.int64)
    print('%d reads of %d letters from both strands (genome %d, 25x), %d candidate pairs, %d with p >= .8 (%d minus)'
          % (R, n, G, len(found), len(keys), int(rev.sum())), flush=True)
    ev = CB.Events(CB.hip_runtime(), 2)
    n_cols = arena.nbytes
    t = dict(old=[], origin=[], both=[])
    ops = 0
    with Pileup(n_cols, L) as p_old, Pileup(n_cols, L, ins_slots=2) as p_new:
        for start, stop, b in aligned_batches(arena, offs, lens, pidx, dr, L, strands=rev, complement=COMP, match_score=1,
                                              mismatch_score=-3, go_score=-5, ge_score=-2):
            ops += int(np.maximum(b.results()['tx_len'], 0).sum())
            kw = dict(mutant_col0=offs[pidx[start:stop, 1]], reverse=rev[start:stop], complement=COMP)
            per = dict(old=[], origin=[], both=[])
            for r in range(3 + args.runs):
                for name, pile, call in (('old', p_old, lambda: b.pileup_add(p_old)), ('origin', p_new, lambda: b.pileup_add(p_new, sides='origin')),
                                         ('both', p_new, lambda: b.pileup_add(p_new, sides='both', **kw))):
                    pile.clear(); b.sync()
                    ev.record(0); call(); ev.record(1)
                    b.sync()
                    if r >= 3:
                        per[name].append(ev.ms(0, 1))
            for name in t:                                         # (several batches: the runs add up batch by batch)
                t[name] = per[name] if not t[name] else [x + y for x, y in zip(t[name], per[name])]
        print('%d ops in %d transcripts' % (ops, len(keys)), flush=True)
        CB.stats('pw_batch_pileup_add (k_pileup_add, origin side)', t['old'], '   %.2f G ops/s' % (ops / (1e6 * float(np.median(t['old'])))))
        CB.stats('pw_batch_pileup_add_sides, origin side, 2 slots', t['origin'], '   %.2f x the old add' % (np.median(t['origin']) / np.median(t['old'])))
        CB.stats('pw_batch_pileup_add_sides, both sides, 2 slots', t['both'], '   %.2f x the old add' % (np.median(t['both']) / np.median(t['old'])))
        letters = np.full(n_cols, 255, np.uint8)
        for o, ln in zip(offs.tolist(), lens.tolist()):
            letters[o:o + ln] = arena[o:o + ln]
        with DeviceArena(letters) as dev:
            tv, tp = [], []
            for r in range(3 + args.runs):
                ev.record(0); p_new.add_letters((dev, 0)); ev.record(1)
                ms = ev.ms(0, 1)
                t0 = time.perf_counter()
                out, offsets, stats = p_new.polish((dev, 0), offs, lens, min_depth=3)
                if r >= 3:
                    tv.append(ms); tp.append(1e3 * (time.perf_counter() - t0))
            CB.stats('pw_pileup_add_letters (%d columns)' % n_cols, tv)
            CB.stats('pw_pileup_polish (%d reads, host wall)' % R, tp)
    ev.close()
    st = {}
    t0 = time.perf_counter()
    got = correct_reads(reads, K, A, .2, .9, p_min=.8, strands='both', complement=COMP, stats=st)
    wall = time.perf_counter() - t0
    print('correct_reads, reads to corrected reads: host wall %.2f s (overlaps: device %.1f ms; vote %.2f ms, alignment and adds %.1f ms, polish %.2f ms); '
          '%d pairs aligned' % (wall, st['overlaps']['device_ms'], st['vote_ms'], st['align_ms'], st['polish_ms'], st['aligned']), flush=True)
    rec = st['records']
    print('columns: kept %d, substituted %d, deleted %d; letters inserted %d' % tuple(int(rec[f].sum()) for f in rec.dtype.names), flush=True)
    m = min(args.eval, R)
    before = sum(edit_distance(reads[r], truth[r]) for r in range(m))
    after = sum(edit_distance(got[r], truth[r]) for r in range(m))
    print('total edit distance to the truth, first %d reads: uncorrected %d, corrected %d' % (m, before, after), flush=True)


if __name__ == '__main__':
    main()
