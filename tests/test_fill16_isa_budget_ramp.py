"""ramp_free and the ISA of config 2's fill kernel `k_fill16<8, false, 3, true>` (no GPU needed).

With ramp_free the steady loop takes the blocks in which diagonals start or end as well (pw_wave.h, WaveFill16::run): it
replaces the feed letters outside the sequences in every block it runs then.  That is
scalar work in front of the unrolled body; it must neither add a loop, nor split the steady body, nor cost a vector
instruction.  Counted as in tests/test_fill16_isa_budget_r5.py: the whole loop of each kind of block.
"""
from tests.test_fill16_isa_budget import DPP_PER_BODY, _valu
from tests.test_fill16_isa_budget_r5 import _loops
from tests.test_fill16_isa_budget_r6 import EDGE_MAX, STEADY_MAX


def test_still_four_loops_within_their_ceilings():
    loops = _loops()
    assert len(loops) == 4
    per_block = [_valu(body) + _valu(close) for body, close in loops]
    print('VALU per block (steady, not started, ended, both):', per_block)
    assert per_block[0] <= STEADY_MAX == 641, per_block
    for got, (kind, ceiling) in zip(per_block[1:], EDGE_MAX.items()):
        assert got <= ceiling, (kind, per_block)


def test_steady_body_is_one_basic_block_with_its_exchanges_and_stores():
    body, close = _loops()[0]
    assert [l for l in body[:-1] if l.startswith(('s_branch', 's_cbranch'))] == []
    assert body[-1].startswith('s_cbranch') and close[-1].startswith('s_branch')
    assert sum(1 for l in body if 'wave_sh' in l) == DPP_PER_BODY == 32
    assert sum(1 for l in body if l.startswith('global_store_dwordx4')) == 2


def test_letter_replacement_in_the_steady_loop_costs_no_vector_select():
    """Replacing the feed letters outside the sequences is arithmetic on wave-uniform values: no vector select in the loop
    (the VALU ceiling above holds the count)."""
    body, close = _loops()[0]
    assert not any(l.startswith('v_cndmask') for l in body + close)
