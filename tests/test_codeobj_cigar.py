"""Tripwire on the compiled CIGAR kernels (pw_cigar.hip; no GPU needed), from the code object's metadata alone: the count and
write kernels keep one wavefront per transcript with everything in registers -- no scratch, no spill, no LDS, no
accumulation registers, 64 VGPRs or fewer (8 wavefronts per SIMD, like K11) -- and the offsets kernel keeps its 1024 chunk sums
in LDS and nothing in scratch."""
import os

from biseqt_amd.csrc import build as B
from biseqt_amd.csrc import codeobj

WAVEFRONT_KERNELS = {'k_cigar_count', 'k_cigar_write', 'k_cigar_count_packed', 'k_cigar_write_packed'}


def test_cigar_kernels_use_no_scratch_and_few_registers():
    path = os.path.join(B.OBJ_DIR, 'pw_cigar.o')
    if not os.path.exists(path):
        B.build()
    md = {n.replace('void ', '').replace('pw::', '').split('(')[0]: k for n, k in codeobj.kernel_metadata(path).items()}
    assert set(md) == WAVEFRONT_KERNELS | {'k_cigar_offsets'}, sorted(md)
    for name, k in md.items():
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (name, k)
        assert k['agpr_count'] == 0, (name, k)
        assert k['vgpr_count'] <= 64, (name, k['vgpr_count'])          # 8 wavefronts per SIMD
        assert k['group_segment_fixed_size'] == (0 if name in WAVEFRONT_KERNELS else 8 * 1024), (name, k)
        assert k['max_flat_workgroup_size'] == (64 if name in WAVEFRONT_KERNELS else 1024), (name, k)
