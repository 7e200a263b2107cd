// pw_fill16p_tu.hip -- config 2's packed fill kernel with its letters read from LDS and ONE running-best key per two cells,
// `k_fill16p<8, false, 3, true>`: rule 3 (scores held times 4), matrix form, 8 diagonals per lane, one pair per wavefront, the
// running best stamped once per four blocks, and which of a key's two cells held the best found out once per pair, in the
// end-cell search (pw_wave.h, WaveFill16, GRP = 4, LDSF, PAIRK).  An object of its own: pw_fill16_bk8_r3_mat.o,
// pw_fill16g_bk8_r3_mat.o and pw_fill16l_bk8_r3_mat.o and their kernels keep their build lines.  Compiled with the flags of those
// objects (build.py).  Exports pw::launch_fill16p_bk8_r3_m1.
#include "pw_device.h"

namespace pw {
hipError_t launch_fill16p_bk8_r3_m1(const FillParams<int32_t>& a, int nwaves, hipStream_t st) {
  hipLaunchKernelGGL((k_fill16p<8, false, 3, true>), dim3((unsigned)nwaves), dim3(64), 0, st, a);
  return hipGetLastError();
}
}  // namespace pw
