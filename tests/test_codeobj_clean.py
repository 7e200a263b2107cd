"""Tripwire on the compiled graph-cleaning kernels (pw_clean.hip; no GPU needed), from the code object's metadata alone: the
object's k_clean_* kernels are exactly the ones DESIGN.md K19 names, none uses scratch, spills, LDS or accumulation
registers, and every one stays within the registers its occupancy needs."""
import os
import re

from biseqt_amd.csrc import build as B
from biseqt_amd.csrc import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The cap is what the design relies on, not the built values: per-vertex and per-arc passes without a software pipeline,
# whose dependent loads (a doubling state behind a vertex, a head's record behind the state, an arc behind a row bound) are
# hidden by other wavefronts only, so all of them must stay at 8 wavefronts per SIMD: 64 VGPRs or fewer.
VGPR_CAP = 64
WORKGROUP = dict.fromkeys(('k_clean_cand', 'k_clean_tips', 'k_clean_bubbles', 'k_clean_drop', 'k_clean_arcs'), 256)


def _design_kernels():
    txt = open(os.path.join(ROOT, 'DESIGN.md')).read()
    k19 = txt[txt.index('### K19 '):txt.index('## 5. Parity')]
    return set(re.findall(r'\bk_clean_\w+', k19))


def test_clean_kernels_are_the_design_s_and_use_no_scratch():
    path = os.path.join(B.OBJ_DIR, 'pw_clean.o')
    if not os.path.exists(path):
        B.build()
    md = {}
    for n, k in codeobj.kernel_metadata(path).items():
        name = n.replace('void ', '').replace('pw::', '').replace('(anonymous namespace)::', '').split('(')[0].split('<')[0]
        if name.startswith('k_clean_'):
            md[name] = k
    assert set(md) == _design_kernels() == set(WORKGROUP), (sorted(md), sorted(_design_kernels()))
    for name, k in md.items():
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (name, k)
        assert k['agpr_count'] == 0 and k['group_segment_fixed_size'] == 0, (name, k)
        assert k['vgpr_count'] <= VGPR_CAP, (name, k['vgpr_count'])
        assert k['max_flat_workgroup_size'] == WORKGROUP[name], (name, k)
