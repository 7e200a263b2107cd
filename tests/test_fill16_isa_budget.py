"""VALU budget of config 2's fill kernel, read from the gfx950 ISA (no GPU needed: the object build.py cross-compiles).

`k_fill16<8, false, 3, true>` (reported as `k_fill16<8, false> x4 matrix`) is bound by vector-ALU issue,
so the count of VALU instructions per 16-step block is what its time follows.  The kernel runs one of four bodies per block
(`WaveFill16::block16<EK>`: steady, diagonals starting, ending, both) and then one shared tail (the key conversion and the
mask stores).  These tests pin:
  * every body is ONE basic block: a branch inside the unrolled body splits it and serialises the packed ops (the edge
    bodies' per-iteration feed range checks used to compile to a branch each);
  * a ceiling on the VALU instructions of the steady block and of every edge block, tail and back edge included.
"""
import collections
import os
import re

from biseqt_amd.csrc import build as B
from biseqt_amd.csrc import codeobj

OBJ = 'pw_fill16_bk8_r3_mat.o'
SYMBOL = '_ZN2pw8k_fill16ILi8ELb0ELi3ELb1EEEvNS_10FillParamsIiEE'
DPP_PER_BODY = 32          # 8 iterations x 4 lane exchanges (origin letter, left offer, mutant letter, up offer)
STEADY_MAX = 690           # was 716 (654 body + 48 tail + 14 back-edge copies)
EDGE_MAX = 920             # was 812, 858 and 954, each body split by a branch per iteration


def _blocks():
    """Basic blocks of the kernel as lists of instruction lines (leaders: branch targets and the instruction after a
    branch)."""
    path = os.path.join(B.OBJ_DIR, OBJ)
    if not os.path.exists(path):
        B.build()
    lines = [l for l in codeobj.disassembly(path, SYMBOL)[SYMBOL] if re.search(r'// [0-9A-Fa-f]+:', l)]
    addr = [int(re.search(r'// ([0-9A-Fa-f]+):', l).group(1), 16) for l in lines]
    base = addr[0]
    leaders = {0}
    for i, l in enumerate(lines):
        if l.startswith(('s_branch', 's_cbranch')):
            m = re.search(r'<%s\+0x([0-9a-f]+)>' % SYMBOL, l)
            if m:
                leaders.add(addr.index(base + int(m.group(1), 16)))
            leaders.add(i + 1)
    cuts = sorted(x for x in leaders if x < len(lines)) + [len(lines)]
    return [[l.split('//')[0].strip() for l in lines[a:b]] for a, b in zip(cuts, cuts[1:])]


def _valu(block):
    return sum(1 for l in block if l.startswith('v_'))


def _bodies_and_tail():
    """The four block bodies, and the instructions every block runs after its body: the tail with the mask stores and
    the loop's back edge (the copies of the loop-carried registers)."""
    blocks = _blocks()
    ib = [i for i, b in enumerate(blocks) if any('wave_sh' in l for l in b)]
    bodies = [blocks[i] for i in ib]
    i = ib[-1] + 1
    while not any(l.startswith('global_store_dwordx4') for l in blocks[i]):
        i += 1
    after = [blocks[i]]
    if blocks[i + 1][-1].startswith('s_branch'):
        after.append(blocks[i + 1])
    return bodies, after


def test_every_block_body_is_one_basic_block():
    bodies, _ = _bodies_and_tail()
    counts = [sum(1 for l in b if 'wave_sh' in l) for b in bodies]
    assert counts == [DPP_PER_BODY] * 4, counts
    for b in bodies:
        inner = [l for l in b[:-1] if l.startswith(('s_branch', 's_cbranch'))]
        assert inner == [], inner


def test_valu_per_block_within_budget():
    bodies, after = _bodies_and_tail()
    tail = sum(_valu(b) for b in after)
    per_block = sorted(_valu(b) + tail for b in bodies)
    steady, edges = per_block[0], per_block[1:]
    assert steady <= STEADY_MAX, (steady, per_block)
    assert max(edges) <= EDGE_MAX, (edges, per_block)


def test_no_copy_of_the_sentinel_in_front_of_a_lane_exchange():
    """The up / left offers shift a loop-carried register onto itself: the edge lane keeps the sentinel without a
    `v_mov` of 0xe000e000 before every DPP move."""
    bodies, _ = _bodies_and_tail()
    for b in bodies:
        ops = collections.Counter(l for l in b if l.startswith('v_mov_b32_e32') and l.endswith('0xe000e000'))
        assert sum(ops.values()) == 0, ops
