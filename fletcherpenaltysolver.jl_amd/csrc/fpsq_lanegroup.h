// fpsq_lanegroup.h -- lanes per row of the CSR row-product kernels: the rule and its compile-time dispatch, shared by the direct
// back-ends (fpsq_direct.hip.h) and the sparse objective Hessian of the iterative handle (fpsq_qp_csr.hip.h).  Host-only.
#pragma once
#include <stdint.h>

namespace fpsq {

// lanes that share a row in the product kernels of the evaluations: the largest power of two <= the mean row length, 1 .. 64
inline int lane_group(int64_t nnz, int64_t rows) {
  const int64_t mean = rows > 0 ? nnz / rows : 1;
  int lg = 1;
  while (lg < 64 && 2 * lg <= mean) lg *= 2;
  return lg;
}

// runs the statement(s) with the compile-time constant LG = lg (a value lane_group returns)
#define WITH_LANE_GROUP(lg, ...)                            \
  switch (lg) {                                             \
    case 1: { constexpr int LG = 1; __VA_ARGS__; } break;    \
    case 2: { constexpr int LG = 2; __VA_ARGS__; } break;    \
    case 4: { constexpr int LG = 4; __VA_ARGS__; } break;    \
    case 8: { constexpr int LG = 8; __VA_ARGS__; } break;    \
    case 16: { constexpr int LG = 16; __VA_ARGS__; } break;  \
    case 32: { constexpr int LG = 32; __VA_ARGS__; } break;  \
    default: { constexpr int LG = 64; __VA_ARGS__; } break;  \
  }

}  // namespace fpsq
