// pw_fill16g_tu.hip -- the grouped form of config 2's packed fill kernel, `k_fill16g<8, false, 3, true>`: rule 3 (scores held
// times 4), matrix form, 8 diagonals per lane, one pair per wavefront, the running best stamped once per four blocks
// (pw_wave.h, WaveFill16, GRP = 4).  An object of its own: pw_fill16_bk8_r3_mat.o and its kernels keep their build line.
// Compiled with the flags of that object (build.py).  Exports pw::launch_fill16g_bk8_r3_m1.
#include "pw_device.h"

namespace pw {
hipError_t launch_fill16g_bk8_r3_m1(const FillParams<int32_t>& a, int nwaves, hipStream_t st) {
  hipLaunchKernelGGL((k_fill16g<8, false, 3, true>), dim3((unsigned)nwaves), dim3(64), 0, st, a);
  return hipGetLastError();
}
}  // namespace pw
