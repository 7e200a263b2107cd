"""Instruction budget of the grouped form of config 2's fill kernel, `k_fill16g<8, false, 3, true>` (pw_wave.h, WaveFill16,
GRP = 4: the running best stamped once per four blocks), read from the gfx950 ISA of its own object (no GPU needed).

The per-block kernel `k_fill16<8, false, 3, true>` issues 641 VALU instructions per steady trip, 24 of them the stamps of
its four key registers (5 each) and the copies of the keys as they stood before the block (1 each).  Here they run once per
four blocks, in a block of their own behind a scalar branch after the mask stores; the position codes of a block's eight
iterations live in scalar registers and move on by a block with 8 scalar adds.  Pinned:
  * ONE loop holds lane exchanges (the kernel is launched for ramp_free batches only), its body one basic block with 32 DPP
    moves and both 16-byte stores, and 32 `v_pk_max_u16` (the four of the stamps are gone from it);
  * the stamp section is a block of its own, entered by a scalar branch at the end of the body;
  * VALU per block: body and closing blocks of the trip that does not stamp, plus a quarter of the stamp section, at most
    641 - 16; the count reached is pinned;
  * scalar instructions of the fast trip (both two-dword feed loads, no stamp): at most 113 + 10;
  * at most 128 VGPRs, no scratch, four wavefronts per SIMD.
"""
import os
import re

from biseqt_amd.csrc import build as B
from biseqt_amd.csrc import codeobj

OBJ = 'pw_fill16g_bk8_r3_mat.o'
SYMBOL = '_ZN2pw9k_fill16gILi8ELb0ELi3ELb1EEEvNS_10FillParamsIiEE'
KERNEL = 'void pw::k_fill16g<8, false, 3, true>('
PARENT_VALU = 641
REQUIRED_VALU_SAVING = 16
VALU_PER_BLOCK_MAX = 623.0          # the count reached: 611 body + 6 closing + 24 / 4
PARENT_SCALAR = 113
SCALAR_ALLOWANCE = 10
FAST_SCALAR_MAX = 116               # the count reached: body 25, the 8 adds of the position codes, closing blocks and headers 83
MAX_VGPRS = 128


def graph():
    """Basic blocks of the kernel: [(instruction lines, successor block indices)]."""
    path = os.path.join(B.OBJ_DIR, OBJ)
    if not os.path.exists(path):
        B.build()
    lines = [l for l in codeobj.disassembly(path, SYMBOL)[SYMBOL] if re.search(r'// [0-9A-Fa-f]+:', l)]
    addr = [int(re.search(r'// ([0-9A-Fa-f]+):', l).group(1), 16) for l in lines]
    text = [l.split('//')[0].strip() for l in lines]
    base = addr[0]
    target = {}
    leaders = {0}
    for i, l in enumerate(text):
        if l.startswith(('s_branch', 's_cbranch')):
            m = re.search(r'<%s\+0x([0-9a-f]+)>' % SYMBOL, lines[i])
            if m:
                target[i] = addr.index(base + int(m.group(1), 16))
                leaders.add(target[i])
            leaders.add(i + 1)
    cuts = sorted(x for x in leaders if x < len(text)) + [len(text)]
    index = {a: n for n, a in enumerate(cuts[:-1])}
    out = []
    for n, (a, b) in enumerate(zip(cuts, cuts[1:])):
        last = text[b - 1]
        succ = []
        if last.startswith(('s_branch', 's_cbranch')) and (b - 1) in target:
            succ.append(index[target[b - 1]])
        if not last.startswith(('s_branch', 's_endpgm')) and b < len(text):
            succ.append(index[b])
        out.append((text[a:b], succ))
    return out


def scalar(block):
    return sum(1 for l in block if l.startswith('s_') and not l.startswith(('s_nop', 's_waitcnt')))


def valu(block):
    return sum(1 for l in block if l.startswith('v_'))


def count(block, op):
    return sum(1 for l in block if l.split()[0] == op)


def cycles(g, start, max_len=24):
    found = []

    def walk(path):
        for s in g[path[-1]][1]:
            if s == start:
                found.append(list(path))
            elif s not in path and len(path) < max_len:
                walk(path + [s])
    walk([start])
    return found


def body_and_stamp(g):
    """(index of the loop body, index of the stamp section): the one block with lane exchanges, and the successor of it that
    holds the stamps' four unsigned maxima."""
    bodies = [n for n, (b, _) in enumerate(g) if any('wave_sh' in l for l in b)]
    assert len(bodies) == 1, bodies
    body = bodies[0]
    assert g[body][0][-1].startswith('s_cbranch_scc'), g[body][0][-1]
    stamps = [s for s in g[body][1] if count(g[s][0], 'v_pk_max_u16') == 4]
    assert len(stamps) == 1 and len(g[body][1]) == 2, (g[body][1], stamps)
    return body, stamps[0]


def fast_cycle(g):
    """The cheapest trip through the body that issues exactly the two two-dword feed loads and does not stamp."""
    body, stamp = body_and_stamp(g)
    ok = []
    for c in cycles(g, body):
        loads = sorted(l.split()[0] for n in c for l in g[n][0] if l.startswith(('s_load', 's_buffer_load')))
        if stamp not in c and loads == ['s_load_dwordx2', 's_load_dwordx2']:
            ok.append(c)
    assert ok, 'no trip with the two two-dword loads'
    return min(ok, key=lambda c: sum(scalar(g[n][0]) for n in c))


def test_one_loop_whose_body_is_one_basic_block():
    g = graph()
    body, _ = body_and_stamp(g)
    b = g[body][0]
    assert [l for l in b[:-1] if l.startswith(('s_branch', 's_cbranch'))] == []
    assert sum(1 for l in b if 'wave_sh' in l) == 32
    assert count(b, 'global_store_dwordx4') == 2
    assert count(b, 'v_pk_max_u16') == 32
    assert not any(l.startswith(('v_readlane', 'v_writelane')) for l in b)


def test_the_stamp_section_is_a_block_of_its_own_behind_a_scalar_branch():
    g = graph()
    body, stamp = body_and_stamp(g)
    s = g[stamp][0]
    assert not any('wave_sh' in l or l.startswith('global_store') for l in s)
    # five ops per key register and the copy of the key: nothing else of the vector ALU
    assert valu(s) == 24, valu(s)
    # the other way round the branch holds no vector work: the position codes move on in scalar registers
    other = [n for n in g[body][1] if n != stamp][0]
    assert valu(g[other][0]) == 0, g[other][0]
    # ... and the stamp section comes back into the loop
    assert any(stamp in c for c in cycles(g, body))


def test_valu_per_block():
    g = graph()
    _, stamp = body_and_stamp(g)
    cyc = fast_cycle(g)
    trip = sum(valu(g[n][0]) for n in cyc)
    per_block = trip + valu(g[stamp][0]) / 4.0
    print('VALU: trip without a stamp %d, stamp section %d, per block %.2f' % (trip, valu(g[stamp][0]), per_block))
    assert per_block <= PARENT_VALU - REQUIRED_VALU_SAVING, per_block
    assert per_block <= VALU_PER_BLOCK_MAX, per_block


def test_fast_path_scalar_count():
    g = graph()
    cyc = fast_cycle(g)
    per_block = [(n, scalar(g[n][0])) for n in cyc]
    total = sum(s for _, s in per_block)
    print('scalar instructions per block of the fast trip (block, count):', per_block, 'total', total)
    assert total <= PARENT_SCALAR + SCALAR_ALLOWANCE, (total, per_block)
    assert total <= FAST_SCALAR_MAX, (total, per_block)
    # the feed loads are still not waited for inside the trip that issues them
    trip = [l for n in cyc for l in g[n][0]]
    first = next(i for i, l in enumerate(trip) if l.startswith('s_load_dwordx2'))
    assert first >= len(g[cyc[0]][0]), 'a feed load inside the body'
    assert [l for l in trip[first:] if l.startswith('s_waitcnt') and 'lgkmcnt' in l] == []


def test_registers_scratch_and_occupancy():
    md = [v for k, v in codeobj.kernel_metadata(os.path.join(B.OBJ_DIR, OBJ)).items() if k.startswith(KERNEL)]
    assert len(md) == 1
    md = md[0]
    print(md)
    assert md['vgpr_count'] <= MAX_VGPRS, md
    assert md['private_segment_fixed_size'] == 0 and md.get('vgpr_spill_count', 0) == 0 and md.get('sgpr_spill_count', 0) == 0, md
    assert 512 // ((md['vgpr_count'] + 7) // 8 * 8) >= 4, md
