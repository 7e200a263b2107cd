"""Instruction budget of config 2's fill kernel with its letters read from LDS, `k_fill16l<8, false, 3, true>` (pw_wave.h,
WaveFill16, GRP = 4, LDSF), read from the gfx950 ISA of its own object (no GPU needed).

The grouped kernel `k_fill16g<8, false, 3, true>` issues 623 VALU instructions per 16-step block, 40 of them only to pass the
matrix rows and selector dwords of the letters from lane to lane (16 copies of a feed value, 16 DPP moves, 8 `v_alignbit`),
and about 100 of its 116 scalar instructions per block rebuild those values for the two edge lanes.  Here every lane reads
both from two rings in LDS, restaged once per eight blocks behind the scalar branch of the stamp group.  Pinned:
  * ONE loop holds lane exchanges, its body one basic block with 16 DPP moves (the two offers of each iteration), at most 16
    `v_alignbit`, 16 LDS reads (as `ds_read_b32` or pairs in `ds_read2_b32`), no LDS write and both 16-byte stores;
  * no scalar load anywhere in the loop, so `lgkmcnt` counts LDS reads only;
  * the stamp section is entered by a scalar branch at the end of the body, the restage section by a scalar branch inside
    it; the restage section holds the LDS writes, the two byte loads of the next chunk and no lane exchange;
  * VALU per block -- the trip that neither stamps nor restages, a quarter of the stamp section, an eighth of the restage
    section: at most the count reached, which is below the grouped kernel's 623 by at least 24;
  * scalar instructions of that trip: at most the count reached, far below the grouped kernel's 116;
  * at most 85 VGPRs, no scratch, LDS small enough for 24 workgroups per CU (160 KiB).
"""
import os
import re

from biseqt_amd.csrc import build as B
from biseqt_amd.csrc import codeobj

OBJ = 'pw_fill16l_bk8_r3_mat.o'
SYMBOL = '_ZN2pw9k_fill16lILi8ELb0ELi3ELb1EEEvNS_10FillParamsIiEE'
KERNEL = 'void pw::k_fill16l<8, false, 3, true>('
GROUPED_VALU = 623
REQUIRED_VALU_SAVING = 24
VALU_PER_BLOCK_MAX = 593.5          # the count reached: 575 body + 9 closing + 24 / 4 + 28 / 8
GROUPED_SCALAR = 116
FAST_SCALAR_MAX = 15                # the count reached: body 3, the 8 adds of the position codes, closing block 4
MAX_VGPRS = 85
MAX_LDS_BYTES = 160 * 1024 // 24


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


def lds_reads(block):
    return count(block, 'ds_read_b32') + 2 * count(block, 'ds_read2_b32')


def lds_writes(block):
    return sum(1 for l in block if l.startswith('ds_write'))


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


def sections(g):
    """(loop body, blocks of the cheapest trip, blocks the stamping trip adds, blocks the restaging trip adds): the body is
    the one block with lane exchanges; the restaging trip is the one that writes LDS, the stamping trip the one that
    holds the stamps' four unsigned maxima and writes none."""
    bodies = [n for n, (b, _) in enumerate(g) if any('wave_sh' in l for l in b)]
    assert len(bodies) == 1, bodies
    body = bodies[0]
    assert g[body][0][-1].startswith('s_cbranch_scc'), g[body][0][-1]
    trips = cycles(g, body)

    def has(c, pred):
        return any(pred(g[n][0]) for n in c if n != body)
    plain = [c for c in trips if not has(c, lds_writes) and not has(c, lambda b: count(b, 'v_pk_max_u16'))]
    stamp = [c for c in trips if not has(c, lds_writes) and has(c, lambda b: count(b, 'v_pk_max_u16') == 4)]
    stage = [c for c in trips if has(c, lds_writes) and has(c, lambda b: count(b, 'v_pk_max_u16') == 4)]
    assert plain and stamp and stage, (len(plain), len(stamp), len(stage))
    key = lambda c: sum(valu(g[n][0]) + scalar(g[n][0]) for n in c)
    fast = min(plain, key=key)
    st = min(stamp, key=key)
    rs = min(stage, key=key)
    return body, fast, [n for n in st if n not in fast], [n for n in rs if n not in st]


def test_one_loop_whose_body_is_one_basic_block():
    g = graph()
    body, _, _, _ = sections(g)
    b = g[body][0]
    assert [l for l in b[:-1] if l.startswith(('s_branch', 's_cbranch'))] == []
    assert sum(1 for l in b if 'wave_sh' in l) == 16
    assert sum(1 for l in b if l.startswith('v_alignbit')) <= 16
    assert lds_reads(b) == 16 and lds_writes(b) == 0
    assert count(b, 'global_store_dwordx4') == 2
    assert count(b, 'v_pk_max_u16') == 32
    assert not any(l.startswith(('v_readlane', 'v_writelane', 's_barrier')) for l in b)


def test_no_scalar_load_in_the_loop():
    g = graph()
    body, fast, stamp, stage = sections(g)
    for n in set(fast) | set(stamp) | set(stage):
        assert [l for l in g[n][0] if l.startswith(('s_load', 's_buffer_load'))] == [], (n, g[n][0])


def test_the_restage_section_lies_behind_the_stamp_branch():
    g = graph()
    body, fast, stamp, stage = sections(g)
    assert body in fast and stamp and stage
    assert not any('wave_sh' in l or l.startswith('global_store') for n in stamp + stage for l in g[n][0])
    assert sum(lds_writes(g[n][0]) for n in stamp) == 0
    # the row, the two halves of the selector dword, and each again for the words repeated behind a row's end
    assert 3 <= sum(lds_writes(g[n][0]) for n in stage) <= 6
    assert sum(count(g[n][0], 'global_load_ubyte') for n in stage) == 2
    assert sum(1 for n in stage for l in g[n][0] if l.startswith('global_load')) == 2
    # the trip that does neither: outside the body, the two ring addresses (add, and) and the five ops the grouped kernel's
    # closing block holds too
    assert sum(valu(g[n][0]) for n in fast if n != body) <= 9


def test_valu_per_block():
    g = graph()
    body, fast, stamp, stage = sections(g)
    trip, st, rs = (sum(valu(g[n][0]) for n in c) for c in (fast, stamp, stage))
    per_block = trip + st / 4.0 + rs / 8.0
    print('VALU: plain trip %d, stamp section %d, restage section %d, per block %.2f' % (trip, st, rs, per_block))
    assert per_block <= GROUPED_VALU - REQUIRED_VALU_SAVING, per_block
    assert per_block <= VALU_PER_BLOCK_MAX, per_block


def test_scalar_count_of_the_plain_trip():
    g = graph()
    body, fast, stamp, stage = sections(g)
    per_block = [(n, scalar(g[n][0])) for n in fast]
    total = sum(s for _, s in per_block)
    print('scalar instructions per block of the plain trip (block, count):', per_block, 'total', total,
          '; stamp section', sum(scalar(g[n][0]) for n in stamp), 'restage section', sum(scalar(g[n][0]) for n in stage))
    assert total <= GROUPED_SCALAR // 2, (total, per_block)
    assert total <= FAST_SCALAR_MAX, (total, per_block)


def test_registers_scratch_and_lds():
    md = [v for k, v in codeobj.kernel_metadata(os.path.join(B.OBJ_DIR, OBJ)).items() if k.startswith(KERNEL)]
    assert len(md) == 1
    md = md[0]
    print(md)
    assert md['vgpr_count'] <= MAX_VGPRS, md
    assert md['private_segment_fixed_size'] == 0 and md.get('vgpr_spill_count', 0) == 0 and md.get('sgpr_spill_count', 0) == 0, md
    assert 0 < md['group_segment_fixed_size'] <= MAX_LDS_BYTES, md
