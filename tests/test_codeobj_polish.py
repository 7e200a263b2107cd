"""Tripwire on the compiled read-correction kernels (pw_polish.hip; no GPU needed), from the code object's metadata alone:
the object's k_polish_* kernels are exactly the ones DESIGN.md names, none uses scratch, spills, LDS or accumulation
registers, and k_polish_add keeps one wavefront per pair and side within the registers its occupancy needs.  (The object
also holds rocPRIM's scan kernels; they are not this test's.)"""
import os
import re

from biseqt_amd.csrc import build as B
from biseqt_amd.csrc import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Registers as built: k_polish_add 36, k_polish_letters 6, k_polish_count 23, k_polish_write 30.  The caps are what the design
# relies on, not the built values: k_polish_add hides the latency of its letter loads and of its atomics behind other
# wavefronts only -- it has no software pipeline, as k_pileup_add -- so it must stay at 8 wavefronts per SIMD (64 VGPRs or
# fewer); the other three are streaming passes and are held to the same bound.
VGPR_CAP = {'k_polish_add': 64, 'k_polish_letters': 64, 'k_polish_count': 64, 'k_polish_write': 64}
WORKGROUP = {'k_polish_add': 64, 'k_polish_letters': 256, 'k_polish_count': 64, 'k_polish_write': 64}


def _design_kernels():
    txt = open(os.path.join(ROOT, 'DESIGN.md')).read()
    return set(re.findall(r'\bk_polish_\w+', txt))


def test_polish_kernels_are_the_design_s_and_use_no_scratch():
    path = os.path.join(B.OBJ_DIR, 'pw_polish.o')
    if not os.path.exists(path):
        B.build()
    md = {}
    for n, k in codeobj.kernel_metadata(path).items():
        name = n.replace('void ', '').replace('pw::', '').replace('(anonymous namespace)::', '').split('(')[0].split('<')[0]
        if name.startswith('k_polish_'):
            md[name] = k
    assert set(md) == _design_kernels() == set(VGPR_CAP), (sorted(md), sorted(_design_kernels()))
    for name, k in md.items():
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (name, k)
        assert k['agpr_count'] == 0 and k['group_segment_fixed_size'] == 0, (name, k)
        assert k['vgpr_count'] <= VGPR_CAP[name], (name, k['vgpr_count'])
        assert k['max_flat_workgroup_size'] == WORKGROUP[name], (name, k)
