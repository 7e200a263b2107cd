"""Tripwire on the compiled summary kernels (pw_txsum.hip; no GPU needed): one wavefront per transcript with every partial
result in registers -- no scratch, no spill, no LDS, no accumulation registers -- and the 48-byte record leaving in three
16-byte vector stores."""
import os

from biseqt_amd.csrc import build as B
from biseqt_amd.csrc import codeobj


def test_summary_kernels_use_no_scratch_and_no_lds():
    path = os.path.join(B.OBJ_DIR, 'pw_txsum.o')
    if not os.path.exists(path):
        B.build()
    md = {n.replace('void ', '').replace('pw::', '').split('(')[0]: k for n, k in codeobj.kernel_metadata(path).items()}
    assert set(md) == {'k_tx_summary', 'k_tx_summary_packed'}, sorted(md)
    for name, k in md.items():
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (name, k)
        assert k['group_segment_fixed_size'] == 0 and k['agpr_count'] == 0, (name, k)
        assert k['vgpr_count'] <= 64, (name, k['vgpr_count'])          # 8 wavefronts per SIMD
    for sym, lines in codeobj.disassembly(path, 'k_tx_summary').items():
        stores = [l.split()[0] for l in lines if l.startswith(('global_store', 'flat_store', 'buffer_store'))]
        assert stores == ['global_store_dwordx4'] * 3, (sym, stores)
        assert not any(l.startswith(('global_atomic', 'flat_atomic', 'buffer_atomic', 'ds_')) and not l.startswith(('ds_bpermute', 'ds_swizzle'))
                       for l in lines), sym
