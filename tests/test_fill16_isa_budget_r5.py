"""Round 5 VALU budget of config 2's fill kernel `k_fill16<8, false, 3, true>`, read from the gfx950 ISA (no GPU needed).

Since round 5 every kind of block of this kernel has a loop of its own (`WaveFill16::run()`, `SPLIT`): a loop is the body's
basic block -- the eight unrolled iterations, the stamp of the running best, the mask assembly and the two stores -- plus
the short block that closes it (the back edge), and nothing else runs per block.  So the count here is the WHOLE loop, which is what the launch executes
per 16-step block.  The parent's single loop, counted the same way, ran a 10-instruction head shared by the four bodies, a
26-instruction block in front of the two "ended" bodies, the body, a 55-instruction tail and 14 copies on the back edge:

    whole loop per block      steady   not started   ended   both
    parent                      694        790         854     950
    round 5                     657        753         817     913

(`tests/test_fill16_isa_budget.py` left the head and the 26 out: its 684 / 780 / 818 / 914.)  What went, per steady block: the
14 back-edge copies and 8 of the head (the bodies no longer join); 12 of the key conversion (the key stays the loop-carried
state, the tail only stamps where it rose); 7 of the mask stores' address and select work.  What stayed against the issue's
list: 4 `v_pk_mul_lo_u16` (the key of a block's last cell, 2 H + 0: still one instruction, a multiply instead of a
multiply-add) and 4 copies on the back edge (the key as it stood before the block has to outlive the block, so the key
alternates between two registers; only two blocks per loop trip would close that).  The
ceilings are the counts reached, each 37 below the parent's.
"""
import collections
import re

from tests.test_fill16_isa_budget import DPP_PER_BODY, _blocks, _valu

STEADY_MAX = 657                                # parent 694, counted the same way
EDGE_MAX = {'not started': 753, 'ended': 817, 'both': 913}    # parent 790, 854, 950
BACK_EDGE_COPIES_MAX = 4                        # parent 14


def _loops():
    """[(body block, closing block)] of the four block loops, steady first, then by size."""
    blocks = _blocks()
    out = []
    for i, b in enumerate(blocks):
        if not any('wave_sh' in l for l in b):
            continue
        # the body ends in the loop's exit branch; the block after it copies what the allocator could not leave in place
        # and branches back in front of the body
        assert b[-1].startswith('s_cbranch'), b[-1]
        close = blocks[i + 1]
        assert close[-1].startswith('s_branch'), close[-1]
        out.append((b, close))
    return sorted(out, key=lambda bc: _valu(bc[0]))


def test_four_loops_each_one_basic_block_holding_both_stores():
    loops = _loops()
    assert len(loops) == 4
    for body, close in loops:
        assert sum(1 for l in body if 'wave_sh' in l) == DPP_PER_BODY
        assert [l for l in body[:-1] if l.startswith(('s_branch', 's_cbranch'))] == []
        # the block's two 16-byte mask stores sit in the body itself: no shared tail
        assert sum(1 for l in body if l.startswith('global_store_dwordx4')) == 2
        assert not any(l.startswith(('global_', 'flat_', 'scratch_', 'buffer_')) for l in close), close


def test_valu_per_block_whole_loop():
    loops = _loops()
    per_block = [_valu(body) + _valu(close) for body, close in loops]
    print('VALU per block (steady, not started, ended, both):', per_block)
    assert per_block[0] <= STEADY_MAX, per_block
    for got, (kind, ceiling) in zip(per_block[1:], EDGE_MAX.items()):
        assert got <= ceiling, (kind, per_block)


def test_back_edge_copies():
    for body, close in _loops():
        copies = [l for l in close if l.startswith('v_')]
        assert all(re.match(r'v_mov_b32_e32 v\d+, v\d+$', l) for l in copies), copies
        assert len(copies) <= BACK_EDGE_COPIES_MAX, copies


def test_mask_stores_take_a_scalar_base():
    """One 32-bit offset register and a scalar base per store: no 64-bit address arithmetic, no select of the spare row
    and no flat store in a block."""
    for body, _ in _loops():
        stores = [l for l in body if l.startswith('global_store_dwordx4')]
        assert all(re.match(r'global_store_dwordx4 v\d+, v\[\d+:\d+\], s\[\d+:\d+\]$', l) for l in stores), stores
        ops = collections.Counter(l.split()[0] for l in body)
        assert ops['v_lshl_add_u64'] == 0 and ops['v_cndmask_b32_e32'] == 0 and ops['v_cmp_lt_u64_e32'] == 0, ops
        assert not any(l.startswith('flat_') for l in body)


def test_key_is_carried_not_converted():
    """The steady block neither re-seeds the key from the best (no multiply-add by 2 in front of the body, no shift back
    in the tail) nor turns it into a step: per key register one masked xor, one and, one min, one multiply-add, one max."""
    body, _ = _loops()[0]
    ops = collections.Counter(l.split()[0] for l in body)
    assert ops['v_pk_lshrrev_b16'] == 0, ops
    assert ops['v_pk_sub_i16'] == 0, ops
    assert ops['v_pk_max_u16'] == 32 + 4, ops           # 32 cell pairs, 4 stamps
