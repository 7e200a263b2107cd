"""Pileups on the device (pw_pileup.hip) beside the alternative they replace.

    python tests/micro/pileup_bench.py [--reads N] [--runs R] [--host-repeats K]

Two solved batches at the read-mapping shape of tests/micro/blot_many_bench.py -- 10 000 reads of 250 letters (mutated slices,
.05 / .03 / .03) against one reference of 100 kb, B_LOCAL, 1 / -3 / -5 / -2, each read in a band of 61 diagonals around its
place: 'spread', every read from a place of its own, and 'one window', all reads drawn from the same 250 letters -- every
wavefront adds to the same 250 columns, the contention worst case.  For each, R runs after three untimed ones: device
milliseconds of pw_batch_pileup_add and of pw_pileup_call, each between two HIP events recorded around the call on the default
stream (the pileup is cleared outside the events), medians and minima; the bytes each way of reading the result moves to the
host; and the existing alternative on the same commit -- pw_batch_pack_transcripts, the packed ops and the records
downloaded and piled up with numpy (one vectorised pass: cumulative sums for the columns, bincount for the counts) -- as host
wall seconds beside the wall seconds of add + call + the sites on the host.  The numpy pileup must equal the device's."""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cigar_bench as CB                                  # noqa: E402  (the event helpers)

L = 4


def make(n_reads, one_window):
    """(arena, offs, lens, pairs, bands): read 0 is the reference."""
    from biseqt_amd import synth
    from biseqt_amd.batch import pack_reads
    rng = synth.rng_for(5100)
    ref = synth.rand_seqs(rng, 1, 100000)[0]
    window = int(rng.integers(0, 100000 - 250 + 1))
    reads, bands = [ref], []
    for _ in range(n_reads):
        at = window if one_window else int(rng.integers(0, 100000 - 250 + 1))
        reads.append(synth.mutate(rng, ref[at:at + 250], .05, .03, .03))
        bands.append((at - 30, at + 30))
    arena, offs, lens = pack_reads(reads)
    return arena, offs, lens, np.array([(0, 1 + k) for k in range(n_reads)], np.int64), np.array(bands, np.int64)


def numpy_pileup(n_cols, res, buf, off, frame, m_off, arena):
    """The pileup of packed transcripts on the host, one vectorised pass (the definition of include/pw_pileup.h)."""
    off = off.astype(np.int64)
    lens = np.diff(off)
    ok = (res['status'] & 1).astype(bool) & ((res['status'] & 14) == 0) & (res['tx_len'] > 0)
    pair = np.repeat(np.arange(len(lens)), lens)
    first = off[:-1][pair]
    k = np.arange(len(buf)) - first
    isM, isD, isI = (buf == 77) | (buf == 83), buf == 68, buf == 73
    co, cm = np.cumsum(isM | isD), np.cumsum(isM | isI)
    base_o = np.concatenate([[0], co])[first]
    base_m = np.concatenate([[0], cm])[first]
    o = co - (isM | isD) - base_o                         # o(k), m(k): exclusive within the pair
    m = cm - (isM | isI) - base_m
    col = frame[pair] + res['origin_idx'][pair].astype(np.int64) + o
    keep = ok[pair]
    counts = np.zeros(n_cols * (L + 2), np.int64)
    sel = isM & keep
    letters = arena[m_off[pair][sel] + res['mutant_idx'][pair][sel].astype(np.int64) + m[sel]].astype(np.int64)
    in_alpha = letters < L
    counts += np.bincount((col[sel] * (L + 2) + letters)[in_alpha], minlength=counts.size)
    sel = isD & keep
    counts += np.bincount(col[sel] * (L + 2) + L, minlength=counts.size)
    prev_I = np.concatenate([[False], isI[:-1]]) & (k > 0)
    sel = isI & ~prev_I & keep & (o > 0)
    counts += np.bincount((col[sel] - 1) * (L + 2) + L + 1, minlength=counts.size)
    return counts.reshape(n_cols, L + 2).astype(np.uint32)


def run(name, n_reads, one_window, runs, host_repeats):
    from biseqt_amd import _pwlib as W
    from biseqt_amd.batch import BatchAligner, DeviceArena, Pileup
    arena, offs, lens, pairs, bands = make(n_reads, one_window)
    n_cols = int(lens[0])
    with DeviceArena(arena) as darena, \
            BatchAligner.from_arena(arena, offs, lens, pairs, diag_ranges=bands, device_arena=darena, alphabet_len=L, alnmode=W.BANDED_MODE,
                                    alntype=W.B_LOCAL, match_score=1, mismatch_score=-3, go_score=-5, ge_score=-2) as b, Pileup(n_cols, L) as p:
        b.solve(); b.traceback(); b.sync()
        res = b.results()
        ops = int(np.maximum(res['tx_len'], 0).sum())
        ev = CB.Events(CB.hip_runtime(), 4)
        t_add, t_call = [], []
        ref_dev = (darena, 0)                              # the reference is read 0 of the arena: its letters are on the device
        for r in range(3 + runs):
            p.clear()
            ev.record(0); b.pileup_add(p); ev.record(1)
            ev.record(2); p.call(ref_dev, min_depth=3); ev.record(3)
            b.sync()
            if r >= 3:
                t_add.append(ev.ms(0, 1)); t_call.append(ev.ms(2, 3))
        counts = p.counts()
        depth = counts[:, :L + 1].sum(axis=1)
        print('%s: %d reads of 250 against %d; %s; %d ops in %d transcripts; depth max %d, mean over covered columns %.1f (%d covered)'
              % (name, n_reads, n_cols, b.kernel_name, ops, int((res['tx_len'] > 0).sum()), int(depth.max()),
                 float(depth[depth > 0].mean()), int((depth > 0).sum())), flush=True)
        CB.stats('pw_batch_pileup_add (k_pileup_add)', t_add, '   %.2f G adds/s' % (ops / (1e6 * float(np.median(t_add)))))
        CB.stats('pw_pileup_call (k_pileup_call, %d columns)' % n_cols, t_call)
        print('bytes to the host: counts %d, sites %d; the alternative: packed ops + offsets + records %d'
              % (counts.nbytes, 8 * n_cols, ops + 8 * (b.n + 1) + 32 * b.n), flush=True)
        # host wall seconds, both ways, from a traced batch to the result on the host
        w_dev, w_alt = [], []
        frame, m_off = offs[pairs[:, 0]], offs[pairs[:, 1]]
        for _ in range(host_repeats):
            p.clear(); b.sync()
            t0 = time.perf_counter()
            b.pileup_add(p); p.call(ref_dev, min_depth=3); sites = p.sites()
            w_dev.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            b.pack_transcripts(); buf, off = b.packed(); res2 = b.results()
            alt = numpy_pileup(n_cols, res2, buf, off, frame, m_off, arena)
            w_alt.append(time.perf_counter() - t0)
        assert (alt == p.counts()).all() and (alt == counts).all()
        assert int(sites['depth'].max()) == int(depth.max())
        print('host wall, traced batch -> result on the host: device add + call + sites %s s (median %.5f); pack + download + numpy '
              'pileup %s s (median %.5f)' % (' '.join('%.5f' % w for w in w_dev), float(np.median(w_dev)),
                                            ' '.join('%.4f' % w for w in w_alt), float(np.median(w_alt))), flush=True)
        ev.close()
        return float(np.median(t_add))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=10000)
    ap.add_argument('--runs', type=int, default=25)
    ap.add_argument('--host-repeats', type=int, default=3)
    args = ap.parse_args()
    CB._import_from(os.path.dirname(os.path.dirname(HERE)))
    assert args.runs >= 20, 'the medians are taken over at least 20 runs'
    spread = run('spread', args.reads, False, args.runs, args.host_repeats)
    worst = run('one window', args.reads, True, args.runs, args.host_repeats)
    print('pileup_add, one window / spread: %.2f x' % (worst / spread), flush=True)


if __name__ == '__main__':
    main()
