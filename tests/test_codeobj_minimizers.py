"""Tripwire on the compiled minimizer-sampling kernels (pw_minimizer.h, and K15d of pw_kmers.hip; no GPU needed), from the code
objects' metadata alone: both translation units that index a read set hold the k_mini_* kernels DESIGN.md names, none uses
scratch, spills or accumulation registers, only the selection pass uses LDS -- exactly its tile of order values -- and every
one stays within the registers its occupancy needs."""
import os
import re

import pytest

from biseqt_amd.csrc import build as B
from biseqt_amd.csrc import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Registers as built: count 18, emit 18 / 24 (reverse), starts 14, occ 16.  The cap is what the design relies on: streaming
# passes of one position, row or read per thread whose loads (a dependent chain of binary-search loads, the letters of a
# k-mer) are hidden by other wavefronts only, so each keeps 8 wavefronts per SIMD: 64 VGPRs or fewer (512 / 8), as K14a-f.
VGPR_CAP = 64
# LDS: the tile of the selection pass, 256 order values and a halo of 127 (window 128, the largest) on each side, 8 bytes
# each.  8 workgroups of 256 threads per CU take 8 x 4080 bytes: a fifth of the CU's LDS.
LDS_BYTES = {'k_mini_count': (256 + 2 * 127) * 8}
KERNELS = {'pw_kmers.o': {'k_mini_count', 'k_mini_emit', 'k_mini_starts', 'k_mini_occ'},
           'pw_overlap.o': {'k_mini_count', 'k_mini_emit', 'k_mini_starts'}}


def _design_kernels():
    txt = open(os.path.join(ROOT, 'DESIGN.md')).read()
    return set(re.findall(r'\bk_mini_\w+', txt))


@pytest.mark.parametrize('obj', sorted(KERNELS))
def test_minimizer_kernels_are_the_design_s_and_use_no_scratch(obj):
    path = os.path.join(B.OBJ_DIR, obj)
    if not os.path.exists(path):
        B.build()
    md = {}
    for n, k in codeobj.kernel_metadata(path).items():
        name = n.replace('void ', '').replace('(anonymous namespace)::', '').split('(')[0].split('<')[0]
        if name.startswith('k_mini_'):
            md.setdefault(name, []).append(k)
    assert set(md) == KERNELS[obj], sorted(md)
    assert _design_kernels() == KERNELS['pw_kmers.o'], sorted(_design_kernels())
    assert len(md['k_mini_count']) == 2 and len(md['k_mini_emit']) == 2        # plain / canonical order, forward / reverse rows
    for name, variants in md.items():
        for k in variants:
            assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (name, k)
            assert k['agpr_count'] == 0, (name, k)
            assert k['group_segment_fixed_size'] == LDS_BYTES.get(name, 0), (name, k)
            assert k['vgpr_count'] <= VGPR_CAP, (name, k['vgpr_count'])
            assert k['max_flat_workgroup_size'] == 256, (name, k)
