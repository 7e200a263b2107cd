"""What ramp_free (pw_plan.h) is predicted to save on bench.py's config 2 batches: the exact number of blocks each of the
four loops of `k_fill16<8, false, 3, true>` takes without it (tests/ramp_free_cases.py restates the planner's steady
range; tests/test_emu_ramp_free.py holds it to the emulator's block counters), times the VALU instructions per block of
each loop (tests/test_fill16_isa_budget_r6.py).  No GPU needed.

    python tests/micro/ramp_blocks.py [batches]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from biseqt_amd import synth  # noqa: E402
from tests import ramp_free_cases as RC  # noqa: E402

VALU = (641, 737, 801, 897)       # steady, not started, ended, both


def main():
    nbatches = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    for j in range(nbatches):
        origins, mutants = synth.pair_batch(bench.batch_seed(0, j), bench.PAIRS, bench.LENGTH)
        total = [0, 0, 0, 0]
        memo = {}
        for o, m in zip(origins, mutants):
            key = (len(o), len(m))
            if key not in memo:
                memo[key] = RC.block_kinds(key[0], key[1], -bench.RADIUS, bench.RADIUS)
            total = [a + b for a, b in zip(total, memo[key])]
        now = sum(n * v for n, v in zip(total, VALU))
        then = sum(total) * VALU[0]
        print('batch %d (seed %d): %d pairs, blocks steady %d, not started %d, ended %d, both %d (%.1f per pair)'
              % ((j, bench.batch_seed(0, j), len(origins)) + tuple(total) + (sum(total) / len(origins),)))
        print('  block loops, VALU per launch: %.6e with the four loops, %.6e all on the steady body: -%.4e (%.2f %%)'
              % (now, then, now - then, 100.0 * (now - then) / now))


if __name__ == '__main__':
    main()
