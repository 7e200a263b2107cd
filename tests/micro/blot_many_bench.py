"""Query-batched Word-Blot (kernels K10 of pw_qseeds.hip) against the loop over the per-query path: one JSON line per shape.

    python tests/micro/blot_many_bench.py [--shapes ig,map] [--queries N] [--repeats R] [--no-many] [--no-loop] [--no-map]

Shapes:
  ig   the Ig-genotyping flow (experiments/blot_ig_genotyping.py:50-76): a reference of 300 letters, 415 queries of about
       300 letters (half of them mutated copies of the reference, half unrelated), wordlen 8, K_min 100;
  map  read mapping: a reference of 100 kb, 10 000 queries of 250 letters (nine in ten a mutated slice of the reference),
       wordlen 12, K_min 100.
Each line: the host wall seconds of WordBlotLocalRef.similar_segments_many (every repeat, the smallest and the median), of the loop
over similar_segments on the same object -- the path without this index; at the map shape on a sample of 500 queries, scaled
to all of them, and the line says so -- the device milliseconds of the batched build / graph / components / box counts
(HIP events of the last call), the hook rounds of the components, and the wall seconds of pipeline.map_queries.  Everything
runs once untimed first (code objects, pools); wall clocks end after the results are on the host.  --queries overrides the
number of queries (for launch counts under rocprofv3 --kernel-trace: they must not depend on it); --no-many /
--no-loop / --no-map leave the batched call (and with it the loop) / the loop / map_queries out.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from biseqt_amd import synth                              # noqa: E402
from biseqt_amd.blot import WordBlotLocalRef              # noqa: E402
from biseqt_amd.pipeline import map_queries               # noqa: E402
from biseqt_amd.sequence import Alphabet, Sequence        # noqa: E402

A = Alphabet('ACGT')
G_MAX, SENS, P_MIN = .2, .99, .7
SHAPES = {'ig': dict(ref=300, queries=415, qlen=300, wordlen=8, K_min=100, related=.5, loop_sample=None),
          'map': dict(ref=100000, queries=10000, qlen=250, wordlen=12, K_min=100, related=.9, loop_sample=500)}


def make(name, n_queries):
    sh = SHAPES[name]
    rng = synth.rng_for(len(name) * 1000 + sh['ref'])
    ref = synth.rand_seqs(rng, 1, sh['ref'])[0]
    queries = []
    for _ in range(n_queries):
        if rng.random() < sh['related']:
            ln = min(sh['qlen'], sh['ref'])
            at = int(rng.integers(0, sh['ref'] - ln + 1))
            queries.append(synth.mutate(rng, ref[at:at + ln], .05, .03, .03))
        else:
            queries.append(synth.rand_seqs(rng, 1, sh['qlen'])[0])
    return Sequence(A, tuple(ref.tolist())), [Sequence(A, tuple(t.tolist())) for t in queries]


def run(name, n_queries, repeats, with_many, with_loop, with_map):
    sh = SHAPES[name]
    n_queries = n_queries or sh['queries']
    ref, queries = make(name, n_queries)
    kw = dict(wordlen=sh['wordlen'], alphabet=A, g_max=G_MAX, sensitivity=SENS)
    K_min = sh['K_min']
    rec = {'shape': name, 'ref_len': len(ref), 'queries': n_queries, 'query_len': sh['qlen'], 'wordlen': sh['wordlen'],
           'K_min': K_min, 'p_min': P_MIN}
    if with_many:
        rec.update(run_many(sh, ref, queries, kw, repeats, with_loop))
    if with_map:
        map_queries(ref, queries[:8], K_min, P_MIN, sh['wordlen'], G_MAX, SENS)            # warm-up of the batch kernels
        t0 = time.perf_counter()
        mapped = map_queries(ref, queries, K_min, P_MIN, sh['wordlen'], G_MAX, SENS)
        rec.update(map_queries_wall_s=round(time.perf_counter() - t0, 5),
                   alignments=sum(r['alignment'] is not None for recs in mapped for r in recs))
    return rec


def run_many(sh, ref, queries, kw, repeats, with_loop):
    K_min, n_queries = sh['K_min'], len(queries)
    wb = WordBlotLocalRef(ref, **kw)
    wb.similar_segments_many(queries[:8], K_min, P_MIN)                      # warm-up: code objects, pools
    list(wb.similar_segments(queries[0], K_min, P_MIN))
    many_s = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        got = wb.similar_segments_many(queries, K_min, P_MIN)
        many_s.append(time.perf_counter() - t0)
    ms = wb.batched_timings()
    rec = {'rows': int(wb._qidx.num_rows()), 'segments': sum(len(g) for g in got),
           'many_wall_s': [round(t, 5) for t in many_s], 'many_wall_s_min': round(min(many_s), 5),
           'many_wall_s_median': round(sorted(many_s)[len(many_s) // 2], 5),
           'build_ms': round(ms['build'], 4), 'graph_ms': round(ms['graph'], 4), 'components_ms': round(ms['components'], 4),
           'counts_ms': round(ms['counts'], 4), 'hook_rounds': ms['rounds']}
    if with_loop:
        sample = queries if not sh['loop_sample'] else queries[:min(sh['loop_sample'], n_queries)]
        loop_s = []
        for _ in range(repeats if not sh['loop_sample'] else 1):
            t0 = time.perf_counter()
            loop = [list(wb.similar_segments(T, K_min, P_MIN)) for T in sample]
            loop_s.append(time.perf_counter() - t0)
        assert all([x['segment'] for x in a] == [x['segment'] for x in b] for a, b in zip(loop, got))
        scale = 1. * n_queries / len(sample)
        rec.update(loop_queries=len(sample), loop_wall_s=[round(t, 5) for t in loop_s],
                   loop_wall_s_scaled_to_all=round(min(loop_s) * scale, 5),
                   loop_note=('measured on all queries' if scale == 1 else
                              'measured on the first %d queries and scaled by %.1f to all %d' % (len(sample), scale, n_queries)),
                   speedup_min_over_min=round(min(loop_s) * scale / min(many_s), 2),
                   speedup_min_loop_over_median_many=round(min(loop_s) * scale / sorted(many_s)[len(many_s) // 2], 2))
    wb.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='ig,map')
    ap.add_argument('--queries', type=int, default=0)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--no-many', action='store_true')
    ap.add_argument('--no-loop', action='store_true')
    ap.add_argument('--no-map', action='store_true')
    args = ap.parse_args()
    for name in args.shapes.split(','):
        print(json.dumps(run(name, args.queries, args.repeats, not args.no_many, not args.no_loop, not args.no_map)), flush=True)


if __name__ == '__main__':
    main()
