"""Tripwire on the compiled pileup kernels (pw_pileup.hip; no GPU needed), from the code object's metadata alone: the object
holds exactly the kernels DESIGN.md names, neither uses scratch, spills, LDS or accumulation registers, and k_pileup_add
keeps one wavefront per pair."""
import os
import re

from biseqt_amd.csrc import build as B
from biseqt_amd.csrc import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Registers as built: k_pileup_add 32, k_pileup_call 11.  The caps are what the design relies on, not the built values:
# k_pileup_add hides the latency of its letter loads and of its atomics behind other wavefronts only -- it has no software
# pipeline -- so it must stay at 8 wavefronts per SIMD (64 VGPRs or fewer, like K11 and K12); k_pileup_call is a streaming
# pass of one row per thread and is held to the same bound.
VGPR_CAP = {'k_pileup_add': 64, 'k_pileup_call': 64}
WORKGROUP = {'k_pileup_add': 64, 'k_pileup_call': 256}


def _design_kernels():
    txt = open(os.path.join(ROOT, 'DESIGN.md')).read()
    return set(re.findall(r'\bk_pileup_\w+', txt))


def test_pileup_kernels_are_the_design_s_and_use_no_scratch():
    path = os.path.join(B.OBJ_DIR, 'pw_pileup.o')
    if not os.path.exists(path):
        B.build()
    md = {n.replace('void ', '').replace('pw::', '').split('(')[0]: k for n, k in codeobj.kernel_metadata(path).items()}
    assert set(md) == _design_kernels() == set(VGPR_CAP), (sorted(md), sorted(_design_kernels()))
    for name, k in md.items():
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (name, k)
        assert k['agpr_count'] == 0 and k['group_segment_fixed_size'] == 0, (name, k)
        assert k['vgpr_count'] <= VGPR_CAP[name], (name, k['vgpr_count'])
        assert k['max_flat_workgroup_size'] == WORKGROUP[name], (name, k)
