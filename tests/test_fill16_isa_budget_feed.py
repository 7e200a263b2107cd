"""Scalar budget of the edge-lane feeders in config 2's fill kernel `k_fill16<8, false, 3, true>`, read from the gfx950 ISA
(no GPU needed).

The kernel is bound by instruction issue, and its time follows every instruction a wavefront issues, scalar ones included
(DESIGN.md section 4 K1).  Counted here: the scalar instructions (`s_*` except `s_nop` and `s_waitcnt`) of one trip of the
steady loop on the FAST PATH of the feeders -- the cheapest cycle of basic blocks through the steady body that issues both
two-dword loads (`WaveFill16::feed_issue`), header blocks, body and closing block, taken branches included.

Counted the same way, the parent's cycle (the cheapest one through its steady body that issues its six clamped
`s_load_dword`: it has one path only) is PARENT_SCALAR = 189:

    block                                   parent   now
    header (funnel shifts, letters-outside test; now also the rows of the 8 origin letters)     23 + 3    7 + 59 + 3
    feed_issue (parent: six clamped loads; now: offset, compare, branch, copy, load per sequence)   56      3 + 2 + 3 + 2
    body                                      106      33
    closing block and back edge                 1     1
    whole trip                                189     113

At least 55 fewer are required; the ceiling pinned is the count reached.
"""
import os
import re

from biseqt_amd.csrc import build as B
from biseqt_amd.csrc import codeobj
from tests.test_fill16_isa_budget import OBJ, SYMBOL

PARENT_SCALAR = 189
REQUIRED_SAVING = 55
FAST_SCALAR_MAX = 113                                   # the count reached
STEADY_VALU_MAX = 641
MAX_VGPRS = 128
KERNEL = 'void pw::k_fill16<8, false, 3, true>('


def graph(path=None):
    """Basic blocks of the kernel: [(instruction lines, successor block indices)]."""
    path = path or os.path.join(B.OBJ_DIR, OBJ)
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


def steady_body(g):
    bodies = [n for n, (b, _) in enumerate(g) if any('wave_sh' in l for l in b)]
    return min(bodies, key=lambda n: valu(g[n][0]))


def cycles(g, start, max_len=24):
    """Simple cycles through block `start`, as lists of block indices beginning with it."""
    found = []

    def walk(path):
        for s in g[path[-1]][1]:
            if s == start:
                found.append(list(path))
            elif s not in path and len(path) < max_len:
                walk(path + [s])
    walk([start])
    return found


def loads(g, cyc):
    return [l for n in cyc for l in g[n][0] if l.startswith('s_load') or l.startswith('s_buffer_load')]


def fast_cycle(g, want=('s_load_dwordx2', 's_load_dwordx2')):
    """The cheapest cycle through the steady body whose scalar loads are exactly `want`, body first."""
    body = steady_body(g)
    ok = [c for c in cycles(g, body) if sorted(l.split()[0] for l in loads(g, c)) == sorted(want)]
    assert ok, 'no cycle through the steady body with loads %r' % (want,)
    return min(ok, key=lambda c: sum(scalar(g[n][0]) for n in c))


def test_fast_path_scalar_count():
    g = graph()
    cyc = fast_cycle(g)
    per_block = [(n, scalar(g[n][0])) for n in cyc]
    total = sum(s for _, s in per_block)
    print('scalar instructions per block of the fast cycle (block, count):', per_block, 'total', total)
    assert total <= PARENT_SCALAR - REQUIRED_SAVING, (total, per_block)
    assert total <= FAST_SCALAR_MAX, (total, per_block)


def test_fast_path_issues_two_two_dword_loads_and_waits_for_them_a_block_later():
    g = graph()
    cyc = fast_cycle(g)
    assert [l.split()[0] for l in loads(g, cyc)] == ['s_load_dwordx2', 's_load_dwordx2']
    # one trip as a line of instructions, rotated to begin with the body; the loads sit behind the body (the blocks that
    # close the trip and open the next) -- nothing between the first load and the body's first instruction of the NEXT trip
    # may wait for the scalar-load counter
    trip = [l for n in cyc for l in g[n][0]]
    first = next(i for i, l in enumerate(trip) if l.startswith('s_load_dwordx2'))
    assert first >= len(g[cyc[0]][0]), 'a feed load inside the body'
    waits = [l for l in trip[first:] if l.startswith('s_waitcnt') and 'lgkmcnt' in l]
    assert waits == [], waits


def test_valu_and_body_shape_unchanged():
    g = graph()
    cyc = fast_cycle(g)
    body = g[cyc[0]][0]
    # (the rows of a block's origin letters live in 8 scalar registers across the body; the kernel parks 6 scalars in lanes of
    #  a vector register in front of its loops and behind them -- never in a trip of the loop)
    assert not any(l.startswith(('v_readlane', 'v_writelane')) for n in cyc for l in g[n][0])
    assert sum(valu(g[n][0]) for n in cyc) <= STEADY_VALU_MAX
    assert [l for l in body[:-1] if l.startswith(('s_branch', 's_cbranch'))] == []
    assert sum(1 for l in body if 'wave_sh' in l) == 32
    assert sum(1 for l in body if l.startswith('global_store_dwordx4')) == 2


def test_registers_scratch_and_occupancy():
    md = [v for k, v in codeobj.kernel_metadata(os.path.join(B.OBJ_DIR, OBJ)).items() if k.startswith(KERNEL)]
    assert len(md) == 1
    md = md[0]
    print(md)
    assert md['vgpr_count'] <= MAX_VGPRS, md
    assert md['private_segment_fixed_size'] == 0 and md.get('vgpr_spill_count', 0) == 0, md
    # four wavefronts per SIMD: 512 VGPRs per lane and SIMD, allocated in blocks of 8
    assert 512 // ((md['vgpr_count'] + 7) // 8 * 8) >= 4, md
