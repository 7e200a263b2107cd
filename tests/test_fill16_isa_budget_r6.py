"""Round 6 VALU budget of config 2's fill kernel `k_fill16<8, false, 3, true>`, read from the gfx950 ISA (no GPU needed).

Counted as in tests/test_fill16_isa_budget_r5.py: the whole loop of each kind of block -- body plus the block that closes
it.  Two groups of 8 instructions per block left, both there only because of how a value was encoded:

  * the tie nibbles are collected as KEPT bits (an unsigned saturating c - x per candidate instead of min(x, c)), so the
    8 accumulators go to the mask plane as they are: no `v_sub_u32 0x77777777 - acc`;
  * a mutant letter's selector code is fixed when the letter enters the window (FIXSEL) and the cell pairs alternate the
    operand order of `v_perm_b32`: no `v_add_u32 0x3fffc` on the spliced register, once per iteration.

    whole loop per block      steady   not started   ended   both
    round 5                     657        753         817     913
    round 6                     641        737         801     897

The ceilings are the counts reached, each 16 below round 5's.
"""
from tests.test_fill16_isa_budget import DPP_PER_BODY, _valu
from tests.test_fill16_isa_budget_r5 import _loops

STEADY_MAX = 641                                # round 5: 657
EDGE_MAX = {'not started': 737, 'ended': 801, 'both': 897}    # round 5: 753, 817, 913


def test_valu_per_block_whole_loop():
    loops = _loops()
    assert len(loops) == 4
    per_block = [_valu(body) + _valu(close) for body, close in loops]
    print('VALU per block (steady, not started, ended, both):', per_block)
    assert per_block[0] <= STEADY_MAX, per_block
    for got, (kind, ceiling) in zip(per_block[1:], EDGE_MAX.items()):
        assert got <= ceiling, (kind, per_block)


def test_steady_body_neither_uninverts_nibbles_nor_repairs_selectors():
    body, close = _loops()[0]
    for l in body + close:
        op = l.split()[0]
        assert not (op.startswith('v_sub_u32') and '0x77777777' in l), l
        assert not (op.startswith('v_add_u32') and '0x3fffc' in l), l


def test_steady_body_keeps_its_lane_exchanges_and_stores():
    body, _ = _loops()[0]
    assert sum(1 for l in body if 'wave_sh' in l) == DPP_PER_BODY
    assert sum(1 for l in body if l.startswith('global_store_dwordx4')) == 2
