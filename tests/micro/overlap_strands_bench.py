"""Config 4 with reads from both strands: R synthetic 5 kb reads at 25x coverage, half of them reverse-complemented.

    python tests/micro/overlap_strands_bench.py MODE[,MODE...] [n_reads] [wordlen] [repeats] [cache.npz]

MODE  forward     raw_all_pairs over the reads as given (the unstranded call)
      both        raw_all_pairs(strands='both'): forward a x forward b and forward a x reverse b, a < b
      minus       raw_all_pairs(strands='-')
      workaround  the unstranded call over the reads plus their materialised reverse complements (2R reads)

One JSON line per mode: device ms of every repeat (pw_overlap_last_ms), listed pairs, seeds and the peak device memory
of the call (hipMemGetInfo sampled from a second thread).  `forward` and `workaround` use nothing but the unstranded
entry point, so the same script measures an older build of the library.  cache.npz keeps the generated reads between
processes.
"""
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from biseqt_amd import synth                            # noqa: E402
from biseqt_amd import _pwlib as W                      # noqa: E402
from biseqt_amd.overlap import raw_all_pairs            # noqa: E402

COMP = np.array([3, 2, 1, 0], np.uint8)


def make_reads(R, cache=None):
    if cache and os.path.exists(cache):
        z = np.load(cache)
        arena, offs = z['arena'], z['offs']            # (every z[...] reads the whole array from the file again)
        return [arena[offs[q]:offs[q + 1]] for q in range(R)], z['starts'], z['flips']
    rng = synth.rng_for(4)
    read_len, cov = 5000, 25
    G = R * read_len // cov
    g = synth.rand_seqs(rng, 1, G)[0]
    starts = rng.integers(0, G - read_len, R)
    reads = [synth.mutate(rng, g[s:s + read_len], .05, .025, .025) for s in starts]
    flips = rng.integers(0, 2, R).astype(bool)
    reads = [np.ascontiguousarray(COMP[r[::-1]]) if f else r for r, f in zip(reads, flips)]
    if cache:
        offs = np.zeros(R + 1, np.int64)
        offs[1:] = np.cumsum([len(r) for r in reads])
        np.savez(cache, arena=np.concatenate(reads), offs=offs, starts=starts, flips=flips)
    return reads, starts, flips


class PeakMemory(object):
    """Peak device memory in use while the block runs, sampled every few milliseconds."""

    def __init__(self, lib, device=0):
        self.lib, self.device, self.low, self.stop = lib, device, None, False

    def _free(self):
        import ctypes as C
        free, total = C.c_uint64(), C.c_uint64()
        self.lib.pw_device_memory(self.device, C.byref(free), C.byref(total))
        return free.value

    def __enter__(self):
        self.base = self.low = self._free()
        self.thread = threading.Thread(target=self._poll)
        self.thread.start()
        return self

    def _poll(self):
        while not self.stop:
            self.low = min(self.low, self._free())
            time.sleep(0.003)

    def __exit__(self, *exc):
        self.stop = True
        self.thread.join()
        self.peak_bytes = self.base - self.low


def main():
    modes = sys.argv[1].split(',')
    R = int(sys.argv[2]) if len(sys.argv) > 2 else 5000
    k = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    cache = sys.argv[5] if len(sys.argv) > 5 else None
    lib = W.load()
    reads, starts, flips = make_reads(R, cache)
    raw_all_pairs(reads[:50], k, 4, .2, .9)              # the first call pays for loading the code objects
    cap = 1 << 26
    for mode in modes:
        if mode == 'workaround':
            args, kw = (list(reads) + [np.ascontiguousarray(COMP[r[::-1]]) for r in reads],), {}
        elif mode == 'forward':
            args, kw = (reads,), {}
        else:
            args, kw = (reads,), dict(strands={'both': 'both', 'minus': '-'}[mode], complement=COMP)
        ms, peak = [], 0
        for _ in range(reps):
            with PeakMemory(lib) as mem:
                out = raw_all_pairs(args[0], k, 4, .2, .9, max_pairs=cap, **kw)
            ms.append(round(out[-1], 2)); peak = max(peak, mem.peak_bytes)
        pairs, recs = out[0], out[-2]
        print(json.dumps(dict(mode=mode, library=os.path.basename(W.PWLIB_SO), reads=R, wordlen=k, device_ms=ms, pairs=int(len(pairs)),
                              seeds=int(recs['n_seeds'].sum()), peak_device_gb=round(peak / 2 ** 30, 2))), flush=True)


if __name__ == '__main__':
    main()
