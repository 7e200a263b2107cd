"""Instruction budget of config 2's fill kernel with its lane-crossing offers handed on through LDS,
`k_fill16x<8, false, 3, true>` (pw_wave.h, WaveFill16, GRP = 4, LDSF, PAIRK, XLDS; offer_up / offer_left), read from the gfx950
ISA of its own object (no GPU needed).

The kernel it stands beside, `k_fill16p<8, false, 3, true>`, moves each of the two offers of an iteration with one
`v_mov_b32_dpp` and one `v_alignbit_b32`: 31 of its VALU instructions per 16-step block.  Here a lane stores the two halves of
an offer where their readers want them (`ds_write_b16`, `ds_write_b16_d16_hi`) and takes its register as one `ds_read_b32`.
Pinned, for both directions through LDS (build.py builds that form unless PW_FILL16X_DIRS asks for one direction):
  * ONE loop, its body one basic block that holds both 16-byte stores;
  * in the body no `v_mov_b32_dpp`, no `wave_shr` / `wave_shl`, no `v_alignbit_b32` (the count reached: 0), no `s_barrier`, no
    `v_readlane` / `v_writelane`, no scalar load in the loop;
  * VALU per block -- the trip that neither stamps nor restages, a quarter of the stamp section, an eighth of the restage
    section -- at most the other kernel's count, read from ITS object the same way, minus 28;
  * LDS instructions in the body: the 16 ring reads, 16 reads of an offer and 32 halfword stores, nothing else: 64;
  * no scratch, no spills, at most 96 VGPRs (five wavefronts per SIMD), and the other kernel's LDS plus the two arrays of
    64 + 1 dwords: 4224 + 520 bytes per wavefront, 20 wavefronts per CU: 94 880 bytes of the CU's 160 KiB.
"""
import os
import re

from biseqt_amd.csrc import build as B
from biseqt_amd.csrc import codeobj
from tests import test_fill16_isa_budget_lds as L
from tests import test_fill16_isa_budget_pairs as P

OBJ = 'pw_fill16x_bk8_r3_mat.o'
SYMBOL = '_ZN2pw9k_fill16xILi8ELb0ELi3ELb1EEEvNS_10FillParamsIiEE'
KERNEL = 'void pw::k_fill16x<8, false, 3, true>('
REQUIRED_VALU_SAVING = 28           # both directions (one direction alone: 13)
BODY_ALIGNBITS = 0                  # the count reached
BODY_LDS_READS = 16 + 16            # ring reads + one dword per offer taken
BODY_LDS_WRITES = 32                # two halfwords per offer handed on
OFFER_BYTES = 2 * 65 * 4
MAX_VGPRS = 96                      # 512 registers per SIMD lane, five wavefronts, granules of 8
WAVES_PER_CU = 20

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


def sections(g):
    """As tests/test_fill16_isa_budget_lds.py, sections(), with the body told by what it must hold here: the block with the
    two 16-byte stores of the mask plane (the other kernels' bodies are told by their DPP moves, which this one has none of)."""
    bodies = [n for n, (b, _) in enumerate(g) if L.count(b, 'global_store_dwordx4') == 2]
    assert len(bodies) == 1, bodies
    body = bodies[0]
    assert g[body][0][-1].startswith('s_cbranch_scc'), g[body][0][-1]
    trips = L.cycles(g, body)

    def has(c, pred):
        return any(pred(g[n][0]) for n in c if n != body)
    plain = [c for c in trips if not has(c, L.lds_writes) and not has(c, lambda b: L.count(b, 'v_pk_max_u16'))]
    stamp = [c for c in trips if not has(c, L.lds_writes) and has(c, lambda b: L.count(b, 'v_pk_max_u16') == 4)]
    stage = [c for c in trips if has(c, L.lds_writes) and has(c, lambda b: L.count(b, 'v_pk_max_u16') == 4)]
    assert plain and stamp and stage, (len(plain), len(stamp), len(stage))
    key = lambda c: sum(L.valu(g[n][0]) + L.scalar(g[n][0]) for n in c)
    fast = min(plain, key=key)
    st = min(stamp, key=key)
    rs = min(stage, key=key)
    return body, fast, [n for n in st if n not in fast], [n for n in rs if n not in st]


def per_block(g):
    body, fast, stamp, stage = sections(g)
    trip, st, rs = (sum(L.valu(g[n][0]) for n in c) for c in (fast, stamp, stage))
    return trip + st / 4.0 + rs / 8.0, (trip, st, rs)


def test_one_loop_whose_body_is_one_basic_block():
    g = graph()
    body, fast, stamp, stage = sections(g)
    b = g[body][0]
    assert [l for l in b[:-1] if l.startswith(('s_branch', 's_cbranch'))] == []
    # the cell pairs are in it: 16 unsigned maxima of the pair keys, as in the other kernel's body
    assert P.opcodes(b)['v_pk_max_u16'] == 16
    for n in set(fast) | set(stamp) | set(stage):
        assert [l for l in g[n][0] if l.startswith(('s_load', 's_buffer_load'))] == [], (n, g[n][0])


def test_no_lane_exchange_on_the_vector_alu():
    g = graph()
    b = g[sections(g)[0]][0]
    assert [l for l in b if 'dpp' in l or 'wave_sh' in l] == []
    assert sum(1 for l in b if l.startswith('v_alignbit')) == BODY_ALIGNBITS
    assert not any(l.startswith(('v_readlane', 'v_writelane', 's_barrier', 'ds_bpermute', 'ds_permute', 'ds_swizzle')) for l in b)
    # ... and nowhere else in the loop
    body, fast, stamp, stage = sections(g)
    for n in set(fast) | set(stamp) | set(stage):
        assert [l for l in g[n][0] if 'dpp' in l or 'wave_sh' in l] == [], n
    # the other kernel's body, read the same way, has the 16 moves and the alignbits
    gp = P.graph()
    bp = gp[L.sections(gp)[0]][0]
    assert sum(1 for l in bp if l.startswith('v_mov_b32_dpp')) == 16 and 15 <= sum(1 for l in bp if l.startswith('v_alignbit')) <= 16


def test_lds_instructions_of_the_body():
    g = graph()
    b = g[sections(g)[0]][0]
    ds = [l.split()[0] for l in b if l.startswith('ds_')]
    by = {op: ds.count(op) for op in sorted(set(ds))}
    print('LDS instructions of the body:', by)
    assert L.lds_reads(b) == BODY_LDS_READS, by
    assert by.get('ds_write_b16', 0) == BODY_LDS_WRITES // 2 and by.get('ds_write_b16_d16_hi', 0) == BODY_LDS_WRITES // 2, by
    assert set(by) <= {'ds_read_b32', 'ds_read2_b32', 'ds_write_b16', 'ds_write_b16_d16_hi'}, by
    assert len(ds) == by.get('ds_read_b32', 0) + by.get('ds_read2_b32', 0) + BODY_LDS_WRITES
    # every offer is read from the address its halves were stored around: one register, immediates 2 bytes apart
    offs = lambda op: sorted(set(int(re.search(r'offset:(\d+)', l).group(1)) for l in b if l.split()[0] == op))
    lo, hi = offs('ds_write_b16'), offs('ds_write_b16_d16_hi')
    assert len(lo) == 2 and hi == [o + 2 for o in lo], (lo, hi)
    assert lo[1] - lo[0] == OFFER_BYTES // 2, (lo, hi)


def test_valu_per_block():
    mine, parts = per_block(graph())
    theirs, parts_p = P.per_block(P.graph())
    print('VALU per block: this kernel %.2f (plain trip %d, stamp section %d, restage section %d); k_fill16p %.2f (%d, %d, %d)'
          % ((mine,) + parts + (theirs,) + parts_p))
    assert mine <= theirs - REQUIRED_VALU_SAVING, (mine, theirs)


def test_registers_scratch_and_lds():
    md = [v for k, v in codeobj.kernel_metadata(os.path.join(B.OBJ_DIR, OBJ)).items() if k.startswith(KERNEL)]
    mp = [v for k, v in codeobj.kernel_metadata(os.path.join(B.OBJ_DIR, P.OBJ)).items() if k.startswith(P.KERNEL)]
    assert len(md) == 1 and len(mp) == 1
    md, mp = md[0], mp[0]
    print(md)
    assert md['vgpr_count'] <= MAX_VGPRS, md
    assert md['private_segment_fixed_size'] == 0 and md.get('vgpr_spill_count', 0) == 0 and md.get('sgpr_spill_count', 0) == 0, md
    assert md['group_segment_fixed_size'] == mp['group_segment_fixed_size'] + OFFER_BYTES, (md, mp)
    assert WAVES_PER_CU * md['group_segment_fixed_size'] < 160 * 1024 * 2 // 3, md
