// fpsq_dense.hip.h -- kernels of the dense-block direct back-end alone (fpsq_dense.hip): the Gram product M = A A' on the
// fp64 matrix cores (k_gemm_nt_f64_w16), its diagonal shift (k_dense_diag), the products with the dense A and A' around the
// M-solves (k_dense_gemv*, k_dense_finish_p).  This is the direct back-end of the seam for small / dense problems
// (reference: the dense A A' + tau I contraction of src/model-Fletcherpenaltynlp.jl:478-484).
//
// All matrices are row-major fp64, padded with zeros to multiples of kDB = 128 (rows of A, order of M) and 32 (columns
// of A: whole k-stages of the Gram product); the padded diagonal of M is set to 1 so the factorisation is unaffected.
#pragma once
#include "fpsq_direct.hip.h"

namespace fpsq {

// C (M x N, ldc) = alpha * A (M x K, lda) * B (N x K, ldb)' + beta * C on the fp64 matrix cores.  M, N multiples of 128, K (or
// the k-chunk of a slice, when gridDim.z > 1: slice z writes the plane C + z * zstride) a multiple of 32.
// One workgroup = one 128 x 128 tile of C on SIXTEEN waves, each a 32 x 32 sub-tile (2 x 2 MFMA tiles).  LOWER: only tiles with
// blockIdx.y >= blockIdx.x are computed (symmetric rank-k update of the lower triangle: the Gram product M = A A').
// Fragment maps of v_mfma_f64_16x16x4_f64 (cdna_hip_programming.md section 3): lane l holds A[i = l & 15][k = l >> 4],
// B[k = l >> 4][j = l & 15]; D register r of lane l is D[row = (l >> 4) + 4 r][col = l & 15].
// Why sixteen waves (tools/mfma_probe.hip): one wave issues a v_mfma_f64_16x16x4_f64 only every ~140 cycles (196 when it
// depends on the previous one), whatever the number of independent accumulators; a SIMD reaches its rate only with several
// waves resident (2 per SIMD: 99 cycles per MFMA).  The four-wave kernel of rounds 1-2 (one wave per SIMD, 64 x 64 per wave,
// removed in round 3) took 0.77 ms for the m = 2048 Gram matrix where this one takes 0.55.
// LDS tiles are [row][k] with leading dimension KD + 1 doubles: the banks are 4 bytes wide and a ds_read_b64 is served 16
// lanes at a time, so the 16 rows of an MFMA operand must start 2 banks apart (leading dimension = 1 mod 16) to cover the
// 32 banks once -- KD + 2, two 8-byte banks apart, measured 50 % conflict cycles.  KD = 32 per stage halves the barriers
// of sixteen waves.
constexpr int kW16Kd = 32, kW16Ld = kW16Kd + 1;
constexpr int kW16Lds = 2 * 2 * kDB * kW16Ld * 8;
template <bool LOWER>
__global__ __launch_bounds__(1024) void k_gemm_nt_f64_w16(double* C, int ldc, const double* __restrict__ A, int lda,
                                                          const double* __restrict__ B, int ldb, int K, double alpha,
                                                          double beta, int kchunk = 0, size_t zstride = 0) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (LOWER && bi < bj) return;
  if (kchunk > 0) {
    const int kbeg = (int)blockIdx.z * kchunk;
    K = min(K, kbeg + kchunk) - kbeg;
    if (K < 0) K = 0;
    C += (size_t)blockIdx.z * zstride;
    A += kbeg;
    B += kbeg;
  }
  extern __shared__ __attribute__((aligned(16))) double gsm[];
  constexpr int KD = kW16Kd, LD = kW16Ld;
  double* sA = gsm;                  // [2][128 * LD]
  double* sB = gsm + 2 * kDB * LD;   // [2][128 * LD]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = (wave >> 2) * 32, wc = (wave & 3) * 32;
  const double* Ab = A + (size_t)bi * kDB * lda;
  const double* Bb = B + (size_t)bj * kDB * ldb;
  const int srow = tid >> 3, sk = (tid & 7) * 4;  // staging: four consecutive k of row (t >> 3) for both operands
  f64x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
  f64x2 ra0, ra1, rb0, rb1;
  auto gload = [&](int k0) {
    const f64x2* pa = reinterpret_cast<const f64x2*>(Ab + (size_t)srow * lda + k0 + sk);
    const f64x2* pb = reinterpret_cast<const f64x2*>(Bb + (size_t)srow * ldb + k0 + sk);
    ra0 = pa[0];
    ra1 = pa[1];
    rb0 = pb[0];
    rb1 = pb[1];
  };
  auto lstore = [&](int buf) {
    double* qa = sA + buf * kDB * LD + srow * LD + sk;
    double* qb = sB + buf * kDB * LD + srow * LD + sk;
    qa[0] = ra0[0];
    qa[1] = ra0[1];
    qa[2] = ra1[0];
    qa[3] = ra1[1];
    qb[0] = rb0[0];
    qb[1] = rb0[1];
    qb[2] = rb1[0];
    qb[3] = rb1[1];
  };
  const int fr = lane & 15, fk = lane >> 4;
  int buf = 0;
  if (K > 0) {
    gload(0);
    lstore(0);
  }
  __syncthreads();
  for (int k0 = 0; k0 < K; k0 += KD) {
    const bool more = k0 + KD < K;
    if (more) gload(k0 + KD);
    const double* pa = sA + buf * kDB * LD + (wr + fr) * LD + fk;
    const double* pb = sB + buf * kDB * LD + (wc + fr) * LD + fk;
#pragma unroll
    for (int ks = 0; ks < KD / 4; ++ks) {
      const double a0 = pa[4 * ks], a1 = pa[16 * LD + 4 * ks], b0 = pb[4 * ks], b1 = pb[16 * LD + 4 * ks];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    if (more) lstore(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }
  double* Cb = C + (size_t)(bi * kDB + wr) * ldc + bj * kDB + wc;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double* p = Cb + (size_t)(i * 16 + fk + 4 * r) * ldc + j * 16 + fr;
        const double v = alpha * acc[i][j][r];
        *p = (beta != 0.0) ? v + beta * *p : v;
      }
}

// M[i][i] += delta for i < m; M[i][i] = 1 on the padding
__global__ void k_dense_diag(double* M, int ld, int m, int mpad, double delta) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < mpad) M[(size_t)i * ld + i] = i < m ? M[(size_t)i * ld + i] + delta : 1.0;
}

// y (len rows) = A (rows x cols, lda) x, for NR right-hand sides interleaved [..][NR]; one wave per row.
template <int NR>
__global__ __launch_bounds__(256) void k_dense_gemv(const double* __restrict__ A, int lda, int rows, int cols,
                                                    const double* __restrict__ x, double alpha, const double* yin,
                                                    double beta, double* y) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  double acc[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) acc[r] = 0.0;
  const double* a = A + (size_t)row * lda;
  for (int c = lane; c < cols; c += 64) {
    const double v = a[c];
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] += v * x[(size_t)c * NR + r];
  }
#pragma unroll
  for (int r = 0; r < NR; ++r) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc[r] += __shfl_down(acc[r], off, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < NR; ++r)
      y[(size_t)row * NR + r] = alpha * acc[r] + (beta != 0.0 ? beta * yin[(size_t)row * NR + r] : 0.0);
  }
}

// part[chunk][c][NR] = sum over the chunk's rows of A[i][c] x[i][NR]   (A' x in two deterministic stages: thread per
// column, coalesced across columns; blockIdx.y splits the rows so that the whole chip streams A)
template <int NR>
__global__ __launch_bounds__(256) void k_dense_gemvt_part(const double* __restrict__ A, int lda, int rows, int cols,
                                                          const double* __restrict__ x, double* part, int rows_per_chunk) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  const int i0 = blockIdx.y * rows_per_chunk, i1 = min(rows, i0 + rows_per_chunk);
  double acc[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) acc[r] = 0.0;
  for (int i = i0; i < i1; ++i) {
    const double v = A[(size_t)i * lda + c];
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] += v * x[(size_t)i * NR + r];
  }
#pragma unroll
  for (int r = 0; r < NR; ++r) part[((size_t)blockIdx.y * cols + c) * NR + r] = acc[r];
}

// out0[c] = a0[c] - sum_chunks part[.][c][0];  out1[c] = (a1 ? a1[c] : 0) - sum_chunks part[.][c][1]
__global__ __launch_bounds__(256) void k_dense_finish_p(const double* __restrict__ part, int nchunk, int cols, int n,
                                                        const double* a0, const double* a1, double* out0, double* out1) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  double s0 = 0.0, s1 = 0.0;
  for (int k = 0; k < nchunk; ++k) {
    s0 += part[((size_t)k * cols + c) * 2];
    s1 += part[((size_t)k * cols + c) * 2 + 1];
  }
  out0[c] = a0[c] - s0;
  out1[c] = (a1 ? a1[c] : 0.0) - s1;
}

}  // namespace fpsq
