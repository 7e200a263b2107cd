"""Tripwire on the compiled overlap-graph kernels (pw_graph.hip; no GPU needed), from the code object's metadata alone:
the object's k_graph_* kernels are exactly the ones DESIGN.md names, none uses scratch, spills, LDS or accumulation
registers, and every one stays within the registers its occupancy needs.  (The object also holds rocPRIM's sort, scan and
search kernels; they are not this test's.)"""
import os
import re

from biseqt_amd.csrc import build as B
from biseqt_amd.csrc import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Registers as built: k_graph_reduce 22, k_graph_classify 23, k_graph_arcs 22, every other kernel 16 or fewer.  The cap is
# what the design relies on, not the built values: none of these kernels has a software pipeline -- k_graph_reduce hides its
# dependent loads (a row's bounds, the arc, the binary search in the target keys, the arc it marks) behind other wavefronts
# only, and the per-record and per-vertex passes stream -- so all of them must stay at 8 wavefronts per SIMD: 64 VGPRs or
# fewer.
VGPR_CAP = 64
WORKGROUP = dict.fromkeys(('k_graph_from_batch', 'k_graph_classify', 'k_graph_arc_count', 'k_graph_arcs', 'k_graph_gather', 'k_graph_twins',
                           'k_graph_out', 'k_graph_chain', 'k_graph_chain_init', 'k_graph_double', 'k_graph_cut', 'k_graph_tails',
                           'k_graph_heads', 'k_graph_emit', 'k_graph_contig_count'), 256)
WORKGROUP.update(k_graph_reduce=64, k_graph_contig_write=64)   # one wavefront per vertex / per member


def _design_kernels():
    """The k_graph_* names of DESIGN.md §4 K17 and §8.10.  (§8.4 names three kernels of the seed indexes' point graphs that
    carry the same prefix -- k_graph_keys, k_graph_dstart, k_graph_scan in pw_seeds.hip -- another object's.)"""
    txt = open(os.path.join(ROOT, 'DESIGN.md')).read()
    k17 = txt[txt.index('### K17 '):txt.index('## 5. Parity')] + txt[txt.index('### 8.10 '):txt.index('## 9. Out of scope')]
    return set(re.findall(r'\bk_graph_\w+', k17))


def test_graph_kernels_are_the_design_s_and_use_no_scratch():
    path = os.path.join(B.OBJ_DIR, 'pw_graph.o')
    if not os.path.exists(path):
        B.build()
    md = {}
    for n, k in codeobj.kernel_metadata(path).items():
        name = n.replace('void ', '').replace('pw::', '').replace('(anonymous namespace)::', '').split('(')[0].split('<')[0]
        if name.startswith('k_graph_'):
            md[name] = k
    assert set(md) == _design_kernels() == set(WORKGROUP), (sorted(md), sorted(_design_kernels()))
    for name, k in md.items():
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (name, k)
        assert k['agpr_count'] == 0 and k['group_segment_fixed_size'] == 0, (name, k)
        assert k['vgpr_count'] <= VGPR_CAP, (name, k['vgpr_count'])
        assert k['max_flat_workgroup_size'] == WORKGROUP[name], (name, k)
