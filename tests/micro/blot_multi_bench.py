"""Multiple-sequence Word-Blot (kernels K9 of pw_mseeds.hip): one JSON line per shape.

    python tests/micro/blot_multi_bench.py [--shapes abc]

Each line: rows, directed edges, device ms of the build / graph / components / count_many (HIP events, the last call of
each inside similar_segments), host wall seconds of the whole similar_segments call and of the index build, and the
build's algorithmic bytes over its device time.  Every shape runs once untimed first (the first launch of a kernel
loads its code object).  Shapes:
  (a) the rearrangement simulation of the reference's experiments/multiple_sequence.py:641-690 scaled to 8 individuals
      x 100 regions x 1 kb (every individual a shuffled, mutated copy of the same regions), wordlen 12, g_max .6,
      sensitivity .9, K_min 900, p_min .6;
  (b) 4 x 20 kb unrelated sequences at wordlen 6 (about 2 x 10^6 chance rows: a neighbour-graph stress case);
  (c) 6 x 20 kb sequences sharing 10 kb, wordlen 10 -- the shape the reference's in-memory class did not finish.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from biseqt_amd.blot import WordBlotMultipleFast   # noqa: E402
from biseqt_amd.sequence import Alphabet, Sequence  # noqa: E402

A = Alphabet('ACGT')


def mutate(rng, s, p):
    s = s.copy()
    flip = rng.random(len(s)) < p
    s[flip] = (s[flip] + rng.integers(1, 4, int(flip.sum()))) % 4
    return s


def shape_a(rng):
    regions = [rng.integers(0, 4, 1000) for _ in range(100)]
    return [np.concatenate([mutate(rng, regions[k], .02) for k in rng.permutation(100)]) for _ in range(8)], \
        dict(wordlen=12, g_max=.6, sensitivity=.9), (900, .6)


def shape_b(rng):
    return [rng.integers(0, 4, 20000) for _ in range(4)], dict(wordlen=6, g_max=.2, sensitivity=.9), (100, .8)


def shape_c(rng):
    core = rng.integers(0, 4, 10000)
    out = []
    for _ in range(6):
        pre = int(rng.integers(0, 10000))
        out.append(np.r_[rng.integers(0, 4, pre), mutate(rng, core, .03), rng.integers(0, 4, 10000 - pre)])
    return out, dict(wordlen=10, g_max=.2, sensitivity=.9), (1000, .7)


def run(name, make):
    rng = np.random.default_rng(ord(name))
    raw, kw, (K_min, p_min) = make(rng)
    seqs = [Sequence(A, s.astype(int).tolist()) for s in raw]
    list(WordBlotMultipleFast(*seqs, alphabet=A, **kw).similar_segments(K_min, p_min))    # warm-up: code objects, pools
    t0 = time.perf_counter()
    WB = WordBlotMultipleFast(*seqs, alphabet=A, **kw)
    t_build = time.perf_counter() - t0
    t0 = time.perf_counter()
    segs = list(WB.similar_segments(K_min, p_min))
    t_seg = time.perf_counter() - t0
    ms = WB._idx.timings()
    rows = WB._idx.num_rows()
    return {'shape': name, 'n_seqs': len(seqs), 'lengths': [len(s) for s in seqs], 'wordlen': kw['wordlen'],
            'K_min': K_min, 'p_min': p_min, 'rows': int(rows), 'edges': int(WB._idx._edges or 0), 'segments': len(segs),
            'build_ms': round(ms['build'], 4), 'graph_ms': round(ms['graph'], 4),
            'components_ms': round(ms['components'], 4), 'counts_ms': round(ms['counts'], 4),
            'index_wall_s': round(t_build, 4), 'similar_segments_wall_s': round(t_seg, 4),
            'build_GBps': round(WB._idx.algorithmic_bytes() / (ms['build'] * 1e6), 3) if ms['build'] > 0 else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='abc')
    args = ap.parse_args()
    makers = {'a': shape_a, 'b': shape_b, 'c': shape_c}
    for name in args.shapes:
        print(json.dumps(run(name, makers[name])), flush=True)


if __name__ == '__main__':
    main()
