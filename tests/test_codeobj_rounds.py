"""Tripwire on the compiled kernels of the iterated consensus (pw_rounds.hip; no GPU needed), from the code object's metadata
alone: the object's k_round_* kernels are exactly the ones DESIGN.md K20 names, none uses scratch, spills, LDS or accumulation
registers, every one keeps within 64 VGPRs and has the workgroup size it was designed with.  (The object also holds rocPRIM's
scan kernels; they are not this test's.)"""
import os
import re

from biseqt_amd.csrc import build as B
from biseqt_amd.csrc import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Registers as built: k_round_count 21, k_round_write 16, k_round_task_write 24, the others 6 .. 12.  The cap is what the design
# relies on, not the built values: every kernel is a streaming pass without a software pipeline that hides its loads behind
# other wavefronts only, so it must stay at 8 wavefronts per SIMD (64 VGPRs or fewer).
KERNELS = ('k_round_count', 'k_round_offsets', 'k_round_write', 'k_round_init', 'k_round_remap', 'k_round_lengths',
           'k_round_task_count', 'k_round_task_write')
VGPR_CAP = 64
WORKGROUP = 256                          # one lane per column, read or contig, in workgroups of 256 everywhere


def _design_kernels():
    txt = open(os.path.join(ROOT, 'DESIGN.md')).read()
    return set(re.findall(r'\bk_round_\w+', txt))


def test_round_kernels_are_the_design_s_and_use_no_scratch():
    path = os.path.join(B.OBJ_DIR, 'pw_rounds.o')
    if not os.path.exists(path):
        B.build()
    md = {}
    for n, k in codeobj.kernel_metadata(path).items():
        name = n.replace('void ', '').replace('pw::', '').replace('(anonymous namespace)::', '').split('(')[0].split('<')[0]
        if name.startswith('k_round_'):
            md[name] = k
    assert set(md) == _design_kernels() == set(KERNELS), (sorted(md), sorted(_design_kernels()))
    for name, k in md.items():
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (name, k)
        assert k['agpr_count'] == 0 and k['group_segment_fixed_size'] == 0, (name, k)
        assert k['vgpr_count'] <= VGPR_CAP, (name, k['vgpr_count'])
        assert k['max_flat_workgroup_size'] == WORKGROUP, (name, k)


def test_the_new_unit_adds_no_kernel_to_the_pinned_sets():
    """The per-read polish, the pileup, the consensus layout and the cleaning keep their kernel sets: pw_rounds.o defines none
    with their prefixes."""
    names = ' '.join(codeobj.kernel_metadata(os.path.join(B.OBJ_DIR, 'pw_rounds.o')))
    assert not re.search(r'\bk_(polish|cons|pileup|clean)_\w+', names)
