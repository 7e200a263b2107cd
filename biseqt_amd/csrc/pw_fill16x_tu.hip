// pw_fill16x_tu.hip -- config 2's packed fill kernel with its letters read from LDS, one running-best key per two cells and
// the two offers that cross lanes handed on through LDS, `k_fill16x<8, false, 3, true>`: rule 3 (scores held times 4), matrix
// form, 8 diagonals per lane, one pair per wavefront; what k_fill16p moves with a DPP move and a v_alignbit per offer, a lane
// stores as two halfwords and its neighbour reads back as one dword (pw_wave.h, WaveFill16, GRP = 4, LDSF, PAIRK, XLDS).  An
// object of its own: pw_fill16p_bk8_r3_mat.o and the objects before it and their kernels keep their build lines.  Compiled
// with the flags of those objects (build.py).  Exports pw::launch_fill16x_bk8_r3_m1.
#include "pw_device.h"

namespace pw {
hipError_t launch_fill16x_bk8_r3_m1(const FillParams<int32_t>& a, int nwaves, hipStream_t st) {
  hipLaunchKernelGGL((k_fill16x<8, false, 3, true>), dim3((unsigned)nwaves), dim3(64), 0, st, a);
  return hipGetLastError();
}
}  // namespace pw
