"""Instruction budget of config 2's fill kernel with one running-best key per two cells, `k_fill16p<8, false, 3, true>`
(pw_wave.h, WaveFill16, GRP = 4, LDSF, PAIRK), read from the gfx950 ISA of its own object (no GPU needed).

The kernel it stands beside, `k_fill16l<8, false, 3, true>`, pays one `v_pk_mad_u16` and one `v_pk_max_u16` per cell pair for
the running best: 64 of its VALU instructions per 16-step block.  Here two consecutive cells of a slot share a key: one
`v_pk_max_i16`, one `v_pk_mad_u16` and one `v_pk_max_u16` per register and two iterations -- 48, a saving of 16.  Pinned:
  * ONE loop holds lane exchanges, its body one basic block with 16 DPP moves;
  * 16 `v_pk_max_u16` in the body (32 in the other kernel's) and at most 16 more `v_pk_max_i16` than the other kernel's body;
  * VALU per block -- the trip that neither stamps nor restages, a quarter of the stamp section, an eighth of the restage
    section -- at most the other kernel's count, read from ITS object the same way, minus 14;
  * no scratch, the same LDS size as the other kernel, and VGPRs within five wavefronts per SIMD (at most 96).
"""
import os
import re

from biseqt_amd.csrc import build as B
from biseqt_amd.csrc import codeobj
from tests import test_fill16_isa_budget_lds as L

OBJ = 'pw_fill16p_bk8_r3_mat.o'
SYMBOL = '_ZN2pw9k_fill16pILi8ELb0ELi3ELb1EEEvNS_10FillParamsIiEE'
KERNEL = 'void pw::k_fill16p<8, false, 3, true>('
REQUIRED_VALU_SAVING = 14
MAX_VGPRS = 96                      # 512 registers per SIMD lane, five wavefronts, granules of 8

_G = {}


def graph():
    """Basic blocks of the kernel, as tests/test_fill16_isa_budget_lds.py reads them from the other object."""
    if 'g' in _G:
        return _G['g']
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
    _G['g'] = out
    return out


def per_block(g):
    body, fast, stamp, stage = L.sections(g)
    trip, st, rs = (sum(L.valu(g[n][0]) for n in c) for c in (fast, stamp, stage))
    return trip + st / 4.0 + rs / 8.0, (trip, st, rs)


def opcodes(block):
    out = {}
    for l in block:
        if l.startswith('v_'):
            op = l.split()[0]
            out[op] = out.get(op, 0) + 1
    return out


def test_one_loop_whose_body_is_one_basic_block():
    g = graph()
    body, _, _, _ = L.sections(g)
    b = g[body][0]
    assert [l for l in b[:-1] if l.startswith(('s_branch', 's_cbranch'))] == []
    assert sum(1 for l in b if 'wave_sh' in l) == 16
    assert L.lds_reads(b) == 16 and L.lds_writes(b) == 0
    assert L.count(b, 'global_store_dwordx4') == 2
    assert not any(l.startswith(('v_readlane', 'v_writelane', 's_barrier')) for l in b)


def test_one_key_per_two_cells_in_the_body():
    g, gl = graph(), L.graph()
    b, bl = g[L.sections(g)[0]][0], gl[L.sections(gl)[0]][0]
    mine, theirs = opcodes(b), opcodes(bl)
    print('body, by opcode: this kernel', sorted(mine.items()), '; k_fill16l', sorted(theirs.items()))
    assert theirs['v_pk_max_u16'] == 32 and mine['v_pk_max_u16'] == 16
    assert mine['v_pk_max_i16'] <= theirs['v_pk_max_i16'] + 16
    assert mine['v_pk_mad_u16'] <= theirs['v_pk_mad_u16'] - 16


def test_valu_per_block():
    mine, parts = per_block(graph())
    theirs, parts_l = per_block(L.graph())
    print('VALU per block: this kernel %.2f (plain trip %d, stamp section %d, restage section %d); k_fill16l %.2f (%d, %d, %d)'
          % ((mine,) + parts + (theirs,) + parts_l))
    assert mine <= theirs - REQUIRED_VALU_SAVING, (mine, theirs)


def test_registers_scratch_and_lds():
    md = [v for k, v in codeobj.kernel_metadata(os.path.join(B.OBJ_DIR, OBJ)).items() if k.startswith(KERNEL)]
    ml = [v for k, v in codeobj.kernel_metadata(os.path.join(B.OBJ_DIR, L.OBJ)).items() if k.startswith(L.KERNEL)]
    assert len(md) == 1 and len(ml) == 1
    md, ml = md[0], ml[0]
    print(md)
    assert md['vgpr_count'] <= MAX_VGPRS, md
    assert md['private_segment_fixed_size'] == 0 and md.get('vgpr_spill_count', 0) == 0 and md.get('sgpr_spill_count', 0) == 0, md
    assert md['group_segment_fixed_size'] == ml['group_segment_fixed_size'] > 0, (md, ml)
