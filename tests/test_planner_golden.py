"""Every decision of the host planner pinned: tests/golden/planner_decisions.json.gz holds what `pw_plan_only` chose for a
grid of batches that straddles every threshold the planner tests (tests/golden/make_planner_golden.py).  A change of the
planner that is meant to change no decision must reproduce all of them; one that is meant to change some regenerates the
file and shows the changed records in its diff."""
import gzip
import importlib.util
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _generator():
    spec = importlib.util.spec_from_file_location('make_planner_golden', os.path.join(GOLDEN, 'make_planner_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_planner_decisions_match_the_golden_table():
    G = _generator()
    with gzip.open(os.path.join(GOLDEN, 'planner_decisions.json.gz')) as f:
        recs = json.load(f)
    assert len(recs) > 5000
    bad = []
    for i, r in enumerate(recs):
        got = json.loads(json.dumps(G.plan(r)))
        if got != r['out']:
            bad.append((i, {k: r[k] for k in ('mode', 'type', 'L', 'scores', 'flags', 'env')}, r['shapes'][:3], r['out'], got))
    assert not bad, '%d of %d decisions changed, first: %s' % (len(bad), len(recs), bad[:3])
