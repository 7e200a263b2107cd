"""Strand-aware query-batched Word-Blot (k_qmatch_stranded of pw_qseeds.hip) against what can be done without it: one JSON
line per shape.

    python tests/micro/blot_many_strands_bench.py [--shapes ig,map] [--queries N] [--repeats R]

The shapes are those of tests/micro/blot_many_bench.py with every second read reverse-complemented (reads from both strands
of the molecule).  Three ways, interleaved, R runs each (default 3), each on a host arena packed beforehand:
  both      similar_segments_many(strands='both'): every query listed on both strands over ONE copy of its letters;
  host_rc   the same 2 n entries without the stranded kernel: the reverse complement of every query materialised on the
            host and one unstranded build over forward + reverse complements; the host's reverse-complement and packing
            seconds are reported separately;
  plus      similar_segments_many(strands='+'): the n queries as written (half the positions).
Per way: the wall seconds of every run (the results on the host), and the device milliseconds of the build / graph /
components / box counts of every run (HIP events, batched_timings()).  `both` and `host_rc` must find the same segments.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from biseqt_amd.batch import pack_reads                   # noqa: E402
from biseqt_amd.blot import WordBlotLocalRef              # noqa: E402
from biseqt_amd.sequence import reverse_complement        # noqa: E402
from tests.micro.blot_many_bench import A, G_MAX, P_MIN, SENS, SHAPES, make     # noqa: E402

COMP = [('A', 'T'), ('C', 'G')]


def run(name, n_queries, repeats):
    sh = SHAPES[name]
    n_queries = n_queries or sh['queries']
    ref, queries = make(name, n_queries)
    queries = [reverse_complement(T, COMP) if q % 2 else T for q, T in enumerate(queries)]
    K_min = sh['K_min']
    wb = WordBlotLocalRef(ref, wordlen=sh['wordlen'], alphabet=A, g_max=G_MAX, sensitivity=SENS)
    t0 = time.perf_counter()
    packed = pack_reads(queries)
    pack_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    twice = queries + [reverse_complement(T, COMP) for T in queries]
    rc_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    packed_twice = pack_reads(twice)
    pack_twice_s = time.perf_counter() - t0
    ways = {'both': lambda: wb.similar_segments_many(queries, K_min, P_MIN, arena=packed, strands='both', complement=COMP),
            'host_rc': lambda: wb.similar_segments_many(twice, K_min, P_MIN, arena=packed_twice),
            'plus': lambda: wb.similar_segments_many(queries, K_min, P_MIN, arena=packed)}
    wb.similar_segments_many(queries[:8], K_min, P_MIN, strands='both', complement=COMP)      # warm-up: code objects, pools
    wb.similar_segments_many(queries[:8], K_min, P_MIN)
    rec = {'shape': name, 'ref_len': len(ref), 'queries': n_queries, 'query_len': sh['qlen'], 'wordlen': sh['wordlen'], 'K_min': K_min,
           'p_min': P_MIN, 'pack_n_s': round(pack_s, 5), 'host_rc_s': round(rc_s, 5), 'pack_2n_s': round(pack_twice_s, 5)}
    out = {w: {'wall_s': [], 'build_ms': [], 'graph_ms': [], 'components_ms': [], 'counts_ms': []} for w in ways}
    got = {}
    for _ in range(repeats):
        for w, f in ways.items():
            t0 = time.perf_counter()
            got[w] = f()
            out[w]['wall_s'].append(round(time.perf_counter() - t0, 5))
            ms = wb.batched_timings()
            for key, field in (('build', 'build_ms'), ('graph', 'graph_ms'), ('components', 'components_ms'), ('counts', 'counts_ms')):
                out[w][field].append(round(ms[key], 4))
            out[w]['rows'] = int(wb._qidx.num_rows())
            out[w]['entries'] = int(wb._qidx.num_queries())
    n = len(queries)
    seg = lambda recs: [r['segment'] for r in recs]                                           # noqa: E731
    assert all(seg(got['both'][q]) == seg(got['host_rc'][q]) + seg(got['host_rc'][n + q]) for q in range(n))
    assert all(seg(got['plus'][q]) == seg(got['host_rc'][q]) for q in range(n))
    for w in ways:
        out[w]['segments'] = sum(len(g) for g in got[w])
    rec.update(out)
    wb.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='ig,map')
    ap.add_argument('--queries', type=int, default=0)
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    for name in args.shapes.split(','):
        print(json.dumps(run(name, args.queries, args.repeats)), flush=True)


if __name__ == '__main__':
    main()
