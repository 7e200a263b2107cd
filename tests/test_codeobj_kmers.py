"""Tripwire on the compiled k-mer table kernels (pw_kmers.hip; no GPU needed), from the code object's metadata alone: the
object's k_kmers_* kernels are exactly the ones DESIGN.md names, none uses scratch, spills or accumulation registers, only
the spectrum kernel uses LDS, and every one stays within the registers its occupancy needs.  (The object also holds the
shared read encoders K9a / K9a' of pw_kmer_encode.h and rocPRIM's kernels; they are not this test's.)"""
import os
import re

from biseqt_amd.csrc import build as B
from biseqt_amd.csrc import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Registers as built: tag 3, heads 6, runs 12, spectrum 16, lookup 14, occ 14.  The caps are what the design relies on, not
# the built values: all six are streaming passes of one row, run or query per thread without a software pipeline -- the
# latency of their loads (for K14e / K14f a dependent chain of binary-search loads) and of their atomics is hidden by other
# wavefronts only, so each must keep 8 wavefronts per SIMD: 64 VGPRs or fewer (512 / 8), as the pileup kernels.
VGPR_CAP = {'k_kmers_tag': 64, 'k_kmers_heads': 64, 'k_kmers_runs': 64, 'k_kmers_spectrum': 64, 'k_kmers_lookup': 64, 'k_kmers_occ': 64}
# LDS: the spectrum's 4096 32-bit bins.  8 wavefronts per SIMD are 8 workgroups of 256 threads per CU: 8 x 16 KB = 128 KB of
# the CU's 160 KB -- a larger histogram would take wavefronts away.
LDS_BYTES = {'k_kmers_spectrum': 4096 * 4}


def _design_kernels():
    txt = open(os.path.join(ROOT, 'DESIGN.md')).read()
    return set(re.findall(r'\bk_kmers_\w+', txt))


def test_kmer_kernels_are_the_design_s_and_use_no_scratch():
    path = os.path.join(B.OBJ_DIR, 'pw_kmers.o')
    if not os.path.exists(path):
        B.build()
    md = {}
    for n, k in codeobj.kernel_metadata(path).items():
        name = n.replace('void ', '').replace('(anonymous namespace)::', '').split('(')[0].split('<')[0]
        if name.startswith('k_kmers_'):
            md[name] = k
    assert set(md) == _design_kernels() == set(VGPR_CAP), (sorted(md), sorted(_design_kernels()))
    for name, k in md.items():
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (name, k)
        assert k['agpr_count'] == 0, (name, k)
        assert k['group_segment_fixed_size'] == LDS_BYTES.get(name, 0), (name, k)
        assert k['vgpr_count'] <= VGPR_CAP[name], (name, k['vgpr_count'])
        assert k['max_flat_workgroup_size'] == 256, (name, k)
