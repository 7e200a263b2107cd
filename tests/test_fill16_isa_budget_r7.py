"""Round 7 issue classes of config 2's fill kernel `k_fill16<8, false, 3, true>`, read from the gfx950 ISA (no GPU needed).

Counted as in tests/test_fill16_isa_budget_r5.py: the whole loop of each kind of block.  Round 7 changes no count, it moves
one instruction per cell pair from the 4-cycle issue class to the 2-cycle one (profiles/round1_valu_issue_table.txt): the
diagonal add `H + row byte` of the matrix form is a plain `v_add_u32` instead of a `v_pk_add_u16` (pw_wave.h,
WaveFill16::cellpair: no half of H can carry into its neighbour).  32 cell pairs per block:

    per block, every loop        v_pk_add_u16   v_add_u32   VALU (steady, not started, ended, both)
    parent (round 6)                  64            1        641  737  801  897
    round 7                           32           33        641  737  801  897

The 32 packed adds that stay are `H + ge` of the gap offers: ge is negative and small scores borrow.
"""
import collections

from tests.test_fill16_isa_budget import DPP_PER_BODY, _valu
from tests.test_fill16_isa_budget_r5 import _loops
from tests.test_fill16_isa_budget_r6 import EDGE_MAX, STEADY_MAX

PARENT_PK_ADD_U16 = 64          # in each of the four loops of the parent build (round 6)
PARENT_ADD_U32 = 1
CELL_PAIRS = 32                 # 8 iterations x 2 steps x 2 registers per parity


def _ops(body, close):
    return collections.Counter(l.split()[0] for l in body + close)


def test_diagonal_add_left_the_packed_class_in_every_loop():
    loops = _loops()
    assert len(loops) == 4
    for body, close in loops:
        ops = _ops(body, close)
        pk_add = ops['v_pk_add_u16']
        add32 = ops['v_add_u32_e32'] + ops['v_add_u32_e64']
        print('v_pk_add_u16 %d, v_add_u32 %d, VALU %d' % (pk_add, add32, _valu(body) + _valu(close)))
        assert pk_add <= PARENT_PK_ADD_U16 - CELL_PAIRS, ops
        assert add32 - PARENT_ADD_U32 == PARENT_PK_ADD_U16 - pk_add, ops


def test_totals_stay_within_round_6():
    per_block = [_valu(body) + _valu(close) for body, close in _loops()]
    assert per_block[0] <= STEADY_MAX, per_block
    for got, (kind, ceiling) in zip(per_block[1:], EDGE_MAX.items()):
        assert got <= ceiling, (kind, per_block)
    for body, _ in _loops():
        assert sum(1 for l in body if 'wave_sh' in l) == DPP_PER_BODY
        assert sum(1 for l in body if l.startswith('global_store_dwordx4')) == 2
