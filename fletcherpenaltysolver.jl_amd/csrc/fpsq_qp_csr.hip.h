// fpsq_qp_csr.hip.h -- the sparse symmetric objective Hessian of the device-resident eq-QP model on the ITERATIVE handle
// (fpsq_qp_create_csr): Q = diag(q) + R, R the off-diagonal part in full symmetric row storage (CSR, rows sorted by column).
// Everything the kernels of the Krylov loop and its tail compute with q stays the diagonal part; R enters in launches of its own,
// around theirs ("sparse objective Hessian on the iterative handle"):
//   objgrad   in front:  s = R x,  d_eff = d + s,  partials of -1/2 x's     (the start-up then forms g = q.*x + d_eff = Q x + d and
//                        sum x (q x / 2 + d_eff) = f + 1/2 x'R x: the partials take the surplus back inside the phi reduction)
//             behind the tail (gated like it):   gx = (the tail's gx) - R p2
//   hprod     in front:  Hsv = q .* v + R v      (instead of k_qp_hsv)
//             behind the tail (gated like it):   Hv = (the tail's Hv) - R (v - p1)
// One row-product body, LG = lane_group(nnz(R), n) lanes per row (fpsq_lanegroup.h), three epilogues as template modes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fpsq_kernels.hip.h"  // LaneCtl, block_sum, kBlock
#include "fpsq_lanegroup.h"

namespace fpsq {

enum QrMode : int { QR_FRONT = 0, QR_HSV = 1, QR_SUB = 2 };

struct QrArgs {
  const int32_t *rowptr, *colind;  // R: n + 1 offsets, nnz(R) columns
  const double* vals;
  const double *a, *b;  // the operand: a_j, or a_j - b_j when b != null (QR_SUB on hprod: v - p1)
  const double* in;     // QR_FRONT: d;  QR_HSV: q (out = q .* a + R a);  QR_SUB: the vector the tail has written
  double* out;          // QR_FRONT: d_eff;  QR_HSV: Hsv;  QR_SUB: the caller's gx / Hv  (never aliases `in`: a launch that runs twice
                        //   writes the same bytes twice)
  double *pf, *pz;      // QR_FRONT: pf[workgroup] = its partial of -1/2 x's, pz[workgroup] = 0 (the slot of the same index in the
                        //   array of ||x - xk||^2 partials, which the phi reduction sums to the same length)
  int32_t n;
};

// out[r] = epilogue(sum_k vals[k] * operand[colind[k]]) over the rows of R: a lane group per row walks its (colind, val) pairs
// with stride LG, gathers the operand and reduces inside the group by xor shuffles (a fixed order; no atomics); lane 0 writes the
// row.  Rows without an entry are ordinary rows (sum 0); the last tile may be ragged.  gate0 != null: the launch was enqueued
// speculatively and runs only when both recurrences have ended, like the tail it stands behind.
template <int LG, int MODE>
__global__ __launch_bounds__(kBlock) void k_qp_csr(const QrArgs A, const LaneCtl* gate0, const LaneCtl* gate1) {
  static_assert(kBlock == 256 && LG >= 1 && LG <= 64 && (LG & (LG - 1)) == 0, "a power-of-two lane group inside a wave");
  if (MODE == QR_SUB && gate0 != nullptr && !(gate0->done && gate1->done)) return;
  constexpr int RPB = kBlock / LG;
  const int32_t* __restrict__ rowptr = A.rowptr;
  const int32_t* __restrict__ colind = A.colind;
  const double* __restrict__ vals = A.vals;
  const double* a = A.a;
  const double* b = A.b;
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  const int rows = A.n;
  const int ntiles = (rows + RPB - 1) / RPB;
  double part = 0.0;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int r = tile * RPB + g;
    double s = 0.0;
    if (r < rows) {
      const int e = rowptr[r + 1];
      if (MODE == QR_SUB && b != nullptr) {
        for (int k = rowptr[r] + l; k < e; k += LG) {
          const int c = colind[k];
          s += vals[k] * (a[c] - b[c]);
        }
      } else {
        for (int k = rowptr[r] + l; k < e; k += LG) s += vals[k] * a[colind[k]];
      }
    }
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (l == 0 && r < rows) {
      if (MODE == QR_FRONT) {
        A.out[r] = A.in[r] + s;
        part += -0.5 * a[r] * s;
      } else if (MODE == QR_HSV) {
        A.out[r] = A.in[r] * a[r] + s;
      } else {
        A.out[r] = A.in[r] - s;
      }
    }
  }
  if (MODE == QR_FRONT) {
    __shared__ double red[4];
    const double t = block_sum(part, red);
    if (threadIdx.x == 0) {
      A.pf[blockIdx.x] = t;
      A.pz[blockIdx.x] = 0.0;
    }
  }
}

}  // namespace fpsq
