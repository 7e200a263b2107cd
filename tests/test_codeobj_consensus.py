"""Tripwire on the compiled consensus-layout kernels (pw_consensus.hip; no GPU needed), from the code object's metadata
alone: the object's k_cons_* kernels are exactly the ones DESIGN.md K18 names, none uses scratch, spills, LDS or
accumulation registers, and every one stays within the registers its occupancy needs.  (The object also holds rocPRIM's
scan kernels; they are not this test's.)"""
import os
import re

from biseqt_amd.csrc import build as B
from biseqt_amd.csrc import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Registers as built: k_cons_task_write 24, k_cons_double and k_cons_place 20, every other kernel 14 or fewer.
# The cap is what the design relies on, not the built values: these are streaming kernels without a software pipeline, which
# hide their dependent loads (a record behind its index, a chain state behind its link, a letter behind a read's offset)
# behind other wavefronts only, so all of them must stay at 8 wavefronts per SIMD: 64 VGPRs or fewer.
VGPR_CAP = 64
WORKGROUP = dict.fromkeys(('k_cons_parent', 'k_cons_chain_init', 'k_cons_double', 'k_cons_roots', 'k_cons_place', 'k_cons_contig_pad',
                           'k_cons_task_count', 'k_cons_task_write', 'k_cons_arena_contigs'), 256)
WORKGROUP.update(k_cons_arena_mutants=64)                  # one wavefront per task


def _design_kernels():
    txt = open(os.path.join(ROOT, 'DESIGN.md')).read()
    k18 = txt[txt.index('### K18 '):txt.index('## 5. Parity')]
    return set(re.findall(r'\bk_cons_\w+', k18))


def test_consensus_kernels_are_the_design_s_and_use_no_scratch():
    path = os.path.join(B.OBJ_DIR, 'pw_consensus.o')
    if not os.path.exists(path):
        B.build()
    md = {}
    for n, k in codeobj.kernel_metadata(path).items():
        name = n.replace('void ', '').replace('pw::', '').replace('(anonymous namespace)::', '').split('(')[0].split('<')[0]
        if name.startswith('k_cons_'):
            md[name] = k
    assert set(md) == _design_kernels() == set(WORKGROUP), (sorted(md), sorted(_design_kernels()))
    for name, k in md.items():
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (name, k)
        assert k['agpr_count'] == 0 and k['group_segment_fixed_size'] == 0, (name, k)
        assert k['vgpr_count'] <= VGPR_CAP, (name, k['vgpr_count'])
        assert k['max_flat_workgroup_size'] == WORKGROUP[name], (name, k)
