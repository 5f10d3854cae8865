// The 8-bit encode of flk_export_args (include/flicker_hip.h), one device function for everything that produces or predicts a stored
// byte: the export kernel and the quantised apply kernels (attack.hip), and the quantised instantiation of the uint8 stem (stem_fwd.hip).
#pragma once
#include "flk_internal.h"

// y = x_adv * mul + add; z = y * levels; q = z >= 0 ? min(rint(z), 255) : 0 -- every operation rounded on its own; NaN -> 0
__device__ static inline int encode_q(float v, float mul, float add, float levels) {
  const float z = __fmul_rn(__fadd_rn(__fmul_rn(v, mul), add), levels);
  return z >= 0.f ? (int)fminf(rintf(z), 255.f) : 0;
}
