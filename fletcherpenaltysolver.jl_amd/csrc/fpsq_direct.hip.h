// fpsq_direct.hip.h -- what the dense (fpsq_dense.hip) and the banded (fpsq_band.hip) direct back-end share.  Kernels: the
// Cholesky of a 128 x 128 diagonal block with its inverse (k_potrf_inv128m), the K = 128 products of a factorisation step
// (k_gemm128_lds), the triangular sweeps by steps (k_trsv_step3), in one launch (k_trsv_chain) and for a tile of 16 columns
// (k_trsm_chain16), the pack / unpack of two interleaved right-hand sides, the COO hand-over (k_coo_to_slots).  Host, in
// namespace fpsq_direct at the end of the file: DirectCore, the state both handles derive from, and what surrounds their
// numeric cores -- set-up and tear-down, the sweeps, the begin / end of a call, argument staging, lane groups.
//
// M = A A' + delta I is factored in 128 x 128 blocks of row-major fp64 on the fp64 matrix cores (v_mfma_f64_16x16x4_f64);
// reference: the LDLtSolver path, src/solve_linear_system.jl:206-252.
#pragma once
#include "../../include/fpsq.h"
#include "fpsq_lanegroup.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace fpsq {

constexpr int kDB = 128;      // block size of the Cholesky / GEMM tiles
using f64x4 = __attribute__((ext_vector_type(4))) double;
using f64x2 = __attribute__((ext_vector_type(2))) double;  // (HIP's double2 is a struct: arrays of it stay in scratch)

// Tile addressing of k_gemm128_lds on a BLOCK-BANDED matrix (fpsq_band): 128 x 128 blocks stored contiguously (row
// stride 128), tile (bi, bj) of C at C + bi * ci + bj * cj, tile bi of A at A + bi * a, tile bj of B at B + bj * b.
struct BlockStrides {
  int on = 0;
  size_t a = 0, b = 0, ci = 0, cj = 0;
};

// The K = 128 products of a factorisation step in ONE memory round trip (the default for the panel and the trailing
// update).  A step of the blocked Cholesky is a link of a dependent chain (nb of them dense, m / 128 banded), and the
// staged kernels above pay eight load -> LDS -> barrier round trips for a 128-deep product (27 us for the panel, ~16 us
// for the update, against 2-3 us of matrix-core time per workgroup).  Here a workgroup issues every global load of its
// operand tiles at once -- whole 1 KB rows per wave instruction, 16 bytes per lane --, parks the tiles in LDS row-major
// with leading dimension = 1 mod 16 doubles (129 / 65: the 16 rows of an MFMA operand start two 4-byte banks apart) and
// runs the k-steps from there, SIXTEEN waves of one 16 x 16 tile each (one wave issues an fp64 MFMA only every
// ~140-196 cycles, tools/mfma_probe.hip: four waves of 2 x 2 tiles took 12.5 / 8.7 us per launch).
// (Loading the MFMA fragments straight from global memory, 8 bytes per lane in 32-byte runs, was measured first:
// 18 / 22 us per launch -- the address unit serialises such loads.)
//   MODE 0: trailing update, tile (bi, bj) of 64 x 64, bi >= bj:  C -= A_bi B_bj'      grid (2 rem, 2 rem), waves 4 x 4
//   MODE 1: panel IN PLACE, rows [32 bi, 32 bi + 32):  P <- P X'  (B = X = the 128 x 128 inverse block, lower
//           triangular: a wave sums only the k <= column part); waves 2 (row tiles) x 8 (column tiles); X goes through
//           LDS in two k-halves (the second only for columns >= 64).
constexpr int kG128Ld = 129, kG128LdX = 65;
constexpr int kG128Lds0 = 2 * 64 * kG128Ld * 8;
constexpr int kG128Lds1 = (32 * kG128Ld + 128 * kG128LdX) * 8;
template <int MODE>
__global__ __launch_bounds__(1024) void k_gemm128_lds(double* C, int ldc, const double* A, int lda, const double* B,
                                                      int ldb, BlockStrides bs) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (MODE == 0 && bi < bj) return;
  extern __shared__ __attribute__((aligned(16))) double gsm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  constexpr int LD = kG128Ld;
  if (MODE == 0) {
    double* sA = gsm;
    double* sB = gsm + 64 * LD;
    const int wr = (wave >> 2) * 16, wc = (wave & 3) * 16;
    const int Ib = bi >> 1, Jb = bj >> 1, si = (bi & 1) * 64, sj = (bj & 1) * 64;
    const double* Ab = A + (bs.on ? (size_t)Ib * bs.a : (size_t)Ib * kDB * lda) + (size_t)si * lda;
    const double* Bb = B + (bs.on ? (size_t)Jb * bs.b : (size_t)Jb * kDB * ldb) + (size_t)sj * ldb;
    double* Cb = C + (bs.on ? (size_t)Ib * bs.ci + (size_t)Jb * bs.cj : (size_t)Ib * kDB * ldc + (size_t)Jb * kDB) +
                 (size_t)(si + wr) * ldc + sj + wc;
    f64x2 va[4], vb[4];
    double cold[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      va[u] = *reinterpret_cast<const f64x2*>(Ab + (size_t)(u * 16 + wave) * lda + 2 * lane);
      vb[u] = *reinterpret_cast<const f64x2*>(Bb + (size_t)(u * 16 + wave) * ldb + 2 * lane);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) cold[r] = Cb[(size_t)(fk + 4 * r) * ldc + fr];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      double* qa = sA + (u * 16 + wave) * LD + 2 * lane;
      double* qb = sB + (u * 16 + wave) * LD + 2 * lane;
      qa[0] = va[u][0];
      qa[1] = va[u][1];
      qb[0] = vb[u][0];
      qb[1] = vb[u][1];
    }
    __syncthreads();
    f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    const double* ar = sA + (wr + fr) * LD + fk;
    const double* br = sB + (wc + fr) * LD + fk;
#pragma unroll 4
    for (int s = 0; s < 32; s += 2) {
      const double a0 = ar[4 * s], b0 = br[4 * s], a1 = ar[4 * s + 4], b1 = br[4 * s + 4];
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) Cb[(size_t)(fk + 4 * r) * ldc + fr] = cold[r] - (acc0[r] + acc1[r]);
  } else {
    constexpr int LX = kG128LdX;
    double* sA = gsm;
    double* sX = gsm + 32 * LD;
    const int Ib = bi >> 2, si = (bi & 3) * 32;
    const double* Ab = A + (bs.on ? (size_t)Ib * bs.a : (size_t)Ib * kDB * lda) + (size_t)si * lda;
    double* Cb = C + (bs.on ? (size_t)Ib * bs.ci : (size_t)Ib * kDB * ldc) + (size_t)si * ldc;
    f64x2 va[2], vx[8];
#pragma unroll
    for (int u = 0; u < 2; ++u) va[u] = *reinterpret_cast<const f64x2*>(Ab + (size_t)(u * 16 + wave) * lda + 2 * lane);
#pragma unroll
    for (int u = 0; u < 8; ++u) vx[u] = *reinterpret_cast<const f64x2*>(B + (size_t)(u * 16 + wave) * ldb + 2 * lane);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      double* qa = sA + (u * 16 + wave) * LD + 2 * lane;
      qa[0] = va[u][0];
      qa[1] = va[u][1];
    }
    if (lane < 32) {  // first k-half of X, all rows
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        double* qx = sX + (u * 16 + wave) * LX + 2 * lane;
        qx[0] = vx[u][0];
        qx[1] = vx[u][1];
      }
    }
    __syncthreads();  // (every wave has read its rows of the panel: the stores below cannot overtake a load)
    const int ri = wave & 1, c = wave >> 1;  // row tile, column tile
    f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    const double* ar = sA + (16 * ri + fr) * LD + fk;
    {
      const double* xr = sX + (16 * c + fr) * LX + fk;
      const int lim = min(16, 4 * (c + 1));  // (a multiple of 4) X[j][k] = 0 for k > j
      for (int s = 0; s < lim; s += 2) {
        const double a0 = ar[4 * s], b0 = xr[4 * s], a1 = ar[4 * s + 4], b1 = xr[4 * s + 4];
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc1, 0, 0, 0);
      }
    }
    __syncthreads();
    if (lane >= 32) {  // second k-half of X, rows j >= 64 only, row j - 64 of the buffer
#pragma unroll
      for (int u = 4; u < 8; ++u) {
        double* qx = sX + (u * 16 + wave - 64) * LX + 2 * lane - 64;
        qx[0] = vx[u][0];
        qx[1] = vx[u][1];
      }
    }
    __syncthreads();
    if (c >= 4) {
      const double* xr = sX + (16 * c - 64 + fr) * LX + fk;
      const int lim = 4 * (c + 1) - 16;
      for (int s = 0; s < lim; s += 2) {
        const double a0 = ar[64 + 4 * s], b0 = xr[4 * s], a1 = ar[64 + 4 * s + 4], b1 = xr[4 * s + 4];
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc1, 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) Cb[(size_t)(16 * ri + fk + 4 * r) * ldc + 16 * c + fr] = acc0[r] + acc1[r];
  }
}

// ---- Cholesky of ONE 128 x 128 diagonal block AND the inverse of its factor (one workgroup; the serial heart of the blocked
// factorisation).  One generation is left in the source, the fifth (k_potrf_inv128m, 44 us per block); the others are in
// the git history of rounds 1-2: (1) unblocked in LDS, three 16-wave barriers per column, 274 us; (2, 3) 64 x 64 / 32 x 32
// sub-blocks factored by ONE wave with the rows in registers, ~220 us whatever their arithmetic -- thousands of straight-line
// instructions executed once per call; (4) a ROLLED loop over eight 16-column panels whose only unrolled part is a 16 x 16
// factor routine on v_readlane broadcasts, left-looking panel updates and row substitutions on the LDS copy, X = L^-1 by
// doubling: 104 us.
__device__ __forceinline__ double rdlane(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

#ifdef FPSQ_POTRF_TIMING  // tools/potrf_probe.hip: s_memtime stamps of thread 0 after every phase
#define POTRF_STAMP() do { if (threadIdx.x == 0 && stamps) stamps[nst++] = (long long)__builtin_readcyclecounter(); } while (0)
#define POTRF_TIMING_ARG , long long* stamps
#else
#define POTRF_STAMP() do {} while (0)
#define POTRF_TIMING_ARG
#endif
// ---- the fifth generation: generation 4's scheme with its two GEMM-shaped parts on the matrix cores.  The phase
// probe of generation 4 (profiles/r02_potrf_phase_probe.txt, cycles of 276k): left-looking panel updates 55k (LDS
// bandwidth: 6 reads per 8 FMAs), the 16 x 16 factor routine 8 x 8.1k, row substitutions 8 x 2.8k, doubling inverse 84k,
// load / stores 44k.  Here
//   (a) the panel update is v_mfma_f64_16x16x4_f64 on 16 x 16 tiles read straight from the LDS copy (leading dimension
//       130: the 16 rows x 4 k of an operand fall in distinct banks); wave 0 updates the diagonal tile and goes on to
//       factor it while waves 1-3 update the tiles below -- their work hides behind the serial 16 x 16 routine;
//   (d) the doubling steps T = L21 X11 and X21 = -X22 T are MFMA tile products too (T kept transposed, 32 columns at a
//       time, so both operands of both products are read k-contiguous); entries of the triangular 16 x 16 diagonal
//       sub-blocks of X are selected on load (strictly lower from the transposed store, diagonal from `dinv`, else 0).
// Step (b) also yields the 16 x 16 inverse (see wave_diag16), which turns (c) into an MFMA product as well.
#ifndef FPSQ_POTRF_LD5
#define FPSQ_POTRF_LD5 (kDB + 2)
#endif
constexpr int kPotrfLd5 = FPSQ_POTRF_LD5;
constexpr int kPotrfTld5 = 66;
constexpr int kPotrfLds5 = (kDB * kPotrfLd5 + 32 * kPotrfTld5 + kDB) * 8;

// the 16 x 16 factor routine (one wave, the serial heart of the kernel: 8 x 7.1k of its ~100k cycles).  Lane r < 16 holds
// row r of the tile in registers and column j is eliminated with v_readlane broadcasts of L[c][j].  Lanes 16 .. 31
// compute X16 = L16^-1 ALONGSIDE, for free: lane 16 + c carries column c of X through the same instruction stream (its
// a[r] starts as e_c; at step j its a[j] * rp is X[j][c], and `a[r] -= X[j][c] * L[r][j]` is the same fused multiply-add
// with the same broadcast L[r][j] the factor lanes use).  X16 goes, transposed, to the upper triangle of the tile (where
// the doubling steps expect it) and lets step (c) be a matrix-core product.
// The routine is ISSUE bound, not latency bound (tools/issue_probe.hip, one wave, counter units: an fp64 FMA 6.4, a
// v_readlane_b32 4 in a batch but 8 when the FMA that consumes it follows at once, rsqrt(double) ~100 for ten dependent
// instructions; eliminating TWO columns per link of the dependent chain -- 1 / l22 = rsqrt(a c - b^2) l11, two independent
// reciprocal square roots -- was built and measured: 8.1k per tile against 7.7k).  So it carries few instructions:
//   * no row selects: the registers of a factor lane above its diagonal hold values nobody reads (lane c is read only
//     for columns < c, and only the lower triangle is stored), and the diagonal lane's own a[j] * rp IS the pivot;
//   * a vanishing pivot is a (uniform, rare) branch instead of selects on every column;
//   * the reciprocal square root is v_rsq_f64 + one third-order correction without the special-value tests (d > tol >= 0
//     is finite here);  1 / L[j][j] is the diagonal of the 16 x 16 inverse the lanes 16 .. 31 carry;
//   * the readlanes of a column's updates are issued as a batch ahead of its FMAs, behind the update of column j + 1 and
//     the next pivot's broadcast.
// 7.7k -> 7.1k per tile against the select-based form of round 2 (~900 instructions -> ~760).  Also tried, slower: the tile
// spread over all 64 lanes, 4 columns each, with ds_bpermute fetches (7.0k against the 6.6k of its time); an unnormalised
// elimination (reciprocal square roots at the end: 9.4k); one LDS store of rp by all lanes (same address: 7.7k).
__device__ __forceinline__ double rsqrt_pos(double d) {
  const double y0 = __builtin_amdgcn_rsq(d);  // ~2^-23 relative
  const double e = fma(-(d * y0), y0, 1.0);
  return fma(y0 * e, fma(e, 0.375, 0.5), y0);  // y0 (1 + e / 2 + 3 e^2 / 8): ~e^3
}
__device__ __forceinline__ void wave_diag16(double* L, int LD, int o, int row0, int* info, double tol, double reg,
                                             double* dinv) {
  const int lane = threadIdx.x & 63;
  const int rl = lane & 15;
  const bool inv = (lane >> 4) == 1;
  double a[16];
  {
    const f64x2* row = reinterpret_cast<const f64x2*>(L + (o + rl) * LD + o);  // (16-byte aligned: LD and o are even)
#pragma unroll
    for (int c = 0; c < 16; c += 2) {
      const f64x2 v = row[c / 2];
      a[c] = inv ? (c == rl ? 1.0 : 0.0) : v[0];
      a[c + 1] = inv ? (c + 1 == rl ? 1.0 : 0.0) : v[1];
    }
  }
  const bool dyn = reg > 0.0;
  const double thr = dyn ? tol : 0.0, sub = dyn ? reg : 1.0;  // (a unit pivot keeps the kernel finite when none is set)
  int nbad = 0, first = 0;
  double d = rdlane(a[0], 0);
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (__builtin_expect(!(d > thr), 0)) {
      first = nbad == 0 ? j + 1 : first;
      ++nbad;
      d = sub;
      if (!inv && rl == j) a[j] = sub;
    }
    const double rp = rsqrt_pos(d);
    const double l = a[j] * rp;
    a[j] = l;
    if (j < 15) {
      a[j + 1] = fma(-l, rdlane(l, j + 1), a[j + 1]);
      d = rdlane(a[j + 1], j + 1);
      double sc[16];
#pragma unroll
      for (int c = j + 2; c < 16; ++c) sc[c] = rdlane(l, c);
#pragma unroll
      for (int c = j + 2; c < 16; ++c) a[c] = fma(-l, sc[c], a[c]);
    }
  }
  if (lane < 16) {
#pragma unroll
    for (int c = 0; c < 16; ++c)
      if (c <= lane) L[(o + lane) * LD + o + c] = a[c];  // L16, lower
  } else if (inv) {
    // X16(r, rl), r > rl, transposed into the upper triangle; X16(rl, rl) = 1 * rp_rl, bit for bit, is 1 / L[rl][rl]
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (r >= rl) *(r == rl ? dinv + o + rl : L + (o + rl) * LD + o + r) = a[r];
  }
  if (lane == 0 && nbad) {
    if (dyn) {
      atomicAdd(info + 1, nbad);
    } else {
      // the LOWEST stored row wins, not the first in time: the two elimination chains of the banded factor run this kernel
      // side by side on two streams, and the reported row must not depend on which of them got there first
      const int v = row0 + o + first;
      int old = atomicCAS(info, 0, v);
      while (old != 0 && old > v) {
        const int seen = atomicCAS(info, old, v);
        if (seen == old) break;
        old = seen;
      }
    }
  }
}

// inv / invT are written in their non-zero triangles only: the caller zero-fills both buffers ONCE (at allocation).
// 512 threads: a wave issues an fp64 MFMA only every ~140-196 cycles (tools/mfma_probe.hip), so the MFMA phases want
// more than one wave per SIMD.
constexpr int kPotrfThreads5 = 512;
inline __global__ __launch_bounds__(kPotrfThreads5) void k_potrf_inv128m(double* Mkk, int ld, double* inv, double* invT, int row0,
                                                                  int* info, double tol, double reg POTRF_TIMING_ARG) {
#ifdef FPSQ_POTRF_TIMING
  int nst = 0;
#endif
  POTRF_STAMP();
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* L = sm;
  constexpr int LD = kPotrfLd5;
  constexpr int NW = kPotrfThreads5 / 64;
  double* Tt = sm + kDB * LD;  // Tt[c][row]: 32 columns x 64 rows of the doubling steps' T, transposed
  constexpr int TLD = kPotrfTld5;
  double* dinv = Tt + 32 * TLD;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int fr = lane & 15, fk = lane >> 4;
  const int tr = (tid & 255) >> 4, tc = tid & 15, th = tid >> 8;  // element of a 16 x 16 tile; tiles 2 u + th
  // the 36 lower tiles, every load in flight at once (one HBM round trip for the block)
  {
    double v[18];
#pragma unroll
    for (int u = 0; u < 18; ++u) {
      int t0 = 2 * u, ti0 = 0;
      while ((ti0 + 1) * (ti0 + 2) / 2 <= t0) ++ti0;
      const int tj0 = t0 - ti0 * (ti0 + 1) / 2;
      int t1 = 2 * u + 1, ti1 = 0;
      while ((ti1 + 1) * (ti1 + 2) / 2 <= t1) ++ti1;
      const int tj1 = t1 - ti1 * (ti1 + 1) / 2;
      const int ti = th ? ti1 : ti0, tj = th ? tj1 : tj0;
      v[u] = Mkk[(size_t)(16 * ti + tr) * ld + 16 * tj + tc];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 18; ++u) {
      int t0 = 2 * u, ti0 = 0;
      while ((ti0 + 1) * (ti0 + 2) / 2 <= t0) ++ti0;
      const int tj0 = t0 - ti0 * (ti0 + 1) / 2;
      int t1 = 2 * u + 1, ti1 = 0;
      while ((ti1 + 1) * (ti1 + 2) / 2 <= t1) ++ti1;
      const int tj1 = t1 - ti1 * (ti1 + 1) / 2;
      const int ti = th ? ti1 : ti0, tj = th ? tj1 : tj0;
      L[(16 * ti + tr) * LD + 16 * tj + tc] = v[u];
    }
  }
  __syncthreads();
  POTRF_STAMP();
  // C(rows of tile t, columns cb) -= L[rows, k0 .. k1) L[cb rows, k0 .. k1)'
  auto tile_update = [&](int t, int cb, int k0, int k1) {
    f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    const double* ar = L + (16 * t + fr) * LD + fk;   // A[i = fr][k = fk]
    const double* br = L + (16 * cb + fr) * LD + fk;  // B[k = fk][j = fr] = L[16 cb + j][k]
    for (int k = k0; k < k1; k += 8) {
      const double a0 = ar[k], b0 = br[k], a1 = ar[k + 4], b1 = br[k + 4];
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) L[(16 * t + fk + 4 * r) * LD + 16 * cb + fr] -= acc0[r] + acc1[r];
  };
#pragma unroll 1
  for (int pb = 0; pb < 8; ++pb) {
    const int o = pb * 16;
    if (pb > 0) {  // (a)
      // wave 0 runs the serial part; wave 4 shares its SIMD and stays out of its way (with it busy the 16 x 16 routine
      // took 8.0k instead of 6.6k cycles); the other six waves update the tiles below
      if (wave == 0) {
        tile_update(pb, pb, o - 16, o);  // the diagonal tile: earlier panels were applied one iteration ago (below)
      } else if (wave != 4) {
        const int wi = wave < 4 ? wave - 1 : wave - 2;  // 0 .. 5
        if (wi == 5 && pb < 7) tile_update(pb + 1, pb + 1, 0, o);  // next diagonal tile, the panels before this one
        for (int t = pb + 1 + wi; t < 8; t += 6) tile_update(t, pb, 0, o);
      }
    }
    if (wave == 0) wave_diag16(L, LD, o, row0, info, tol, reg, dinv);  // (b)
    __syncthreads();
    POTRF_STAMP();
    // (c) tiles below: P <- P X16' on the matrix cores.  B[k][j] = X16(j, k): strictly lower entries from the transposed
    // store, the diagonal from dinv, zero above
    for (int t = pb + 1 + wave; t < 8; t += NW) {
      double av[4], bv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = 4 * q + fk;
        av[q] = L[(16 * t + fr) * LD + o + k];
        const double xv = L[(o + k) * LD + o + fr];
        bv[q] = fr > k ? xv : (fr == k ? dinv[o + fr] : 0.0);
      }
      f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[0], bv[0], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[1], bv[1], acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[2], bv[2], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[3], bv[3], acc1, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) L[(16 * t + fk + 4 * r) * LD + o + fr] = acc0[r] + acc1[r];
    }
    __syncthreads();
    POTRF_STAMP();
  }
#pragma unroll
  for (int u = 0; u < 18; ++u) {
    int t0 = 2 * u, ti0 = 0;
    while ((ti0 + 1) * (ti0 + 2) / 2 <= t0) ++ti0;
    const int tj0 = t0 - ti0 * (ti0 + 1) / 2;
    int t1 = 2 * u + 1, ti1 = 0;
    while ((ti1 + 1) * (ti1 + 2) / 2 <= t1) ++ti1;
    const int tj1 = t1 - ti1 * (ti1 + 1) / 2;
    const int ti = th ? ti1 : ti0, tj = th ? tj1 : tj0;
    if (ti != tj || tc <= tr) Mkk[(size_t)(16 * ti + tr) * ld + 16 * tj + tc] = L[(16 * ti + tr) * LD + 16 * tj + tc];
  }
  POTRF_STAMP();
  // (d) X = L^-1 by doubling; X(r, c), r > c, lives at L[c * LD + r] (the 16 x 16 diagonal inverses are there already)
#pragma unroll 1
  for (int h = 16; h < kDB; h *= 2) {
    const int w = h < 32 ? h : 32;
    const int ntile = 4 * (w / 16);  // 64 rows (all pairs of the level) x w columns of T in 16 x 16 tiles
#pragma unroll 1
    for (int cc = 0; cc < h; cc += w) {
      for (int tl = wave; tl < ntile; tl += NW) {  // T[q h + r][c] = sum_{p >= c} L21[r][p] X11(p, c)
        const int gr0 = (tl & 3) * 16, ct = tl >> 2;
        const int q = gr0 / h, r0 = gr0 % h, b0 = q * 2 * h, c0 = cc + ct * 16;
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        const double* arow = L + (b0 + h + r0 + fr) * LD + b0;  // A[i][p] = L21[r0 + i][p]
        const double* bcol = L + (b0 + c0 + fr) * LD + b0;      // B[p][j] = X11(p, c0 + j)
        const double dj = dinv[b0 + c0 + fr];
#pragma unroll
        for (int p0 = 0; p0 < 16; p0 += 4) {
          const int p = c0 + p0 + fk, c = c0 + fr;
          const double a = arow[p];
          const double xv = bcol[p];
          const double b = p > c ? xv : (p == c ? dj : 0.0);
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
        f64x4 acc2 = {0.0, 0.0, 0.0, 0.0};
        for (int p0 = c0 + 16; p0 < h; p0 += 16) {  // (h - c0 is a multiple of 16) operands of four k-steps, then the MFMAs
          double av[4], bv[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            av[u] = arow[p0 + 4 * u + fk];
            bv[u] = bcol[p0 + 4 * u + fk];
          }
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[0], bv[0], acc, 0, 0, 0);
          acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[1], bv[1], acc2, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[2], bv[2], acc, 0, 0, 0);
          acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[3], bv[3], acc2, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) Tt[(ct * 16 + fr) * TLD + gr0 + fk + 4 * r] = acc[r] + acc2[r];
      }
      __syncthreads();
      POTRF_STAMP();
      for (int tl = wave; tl < ntile; tl += NW) {  // X21[r][c] = - sum_{p <= r} X22(r, p) T[p][c]
        const int gr0 = (tl & 3) * 16, ct = tl >> 2;
        const int q = gr0 / h, r0 = gr0 % h, b0 = q * 2 * h;
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        const double* xcol = L + (size_t)(b0 + h) * LD + b0 + h + r0 + fr;  // A[i][p] = X22(r0 + i, p) = xcol[p * LD], p < r0 + i
        const double* tb = Tt + (ct * 16 + fr) * TLD + q * h;               // B[p][j] = T[q h + p][ct 16 + j]
        f64x4 acc2 = {0.0, 0.0, 0.0, 0.0};
        for (int p0 = 0; p0 < r0; p0 += 16) {
          double av[4], bv[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            av[u] = xcol[(p0 + 4 * u + fk) * LD];
            bv[u] = tb[p0 + 4 * u + fk];
          }
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[0], bv[0], acc, 0, 0, 0);
          acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[1], bv[1], acc2, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[2], bv[2], acc, 0, 0, 0);
          acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[3], bv[3], acc2, 0, 0, 0);
        }
#pragma unroll
        for (int p0 = 0; p0 < 16; p0 += 4) {
          const int p = r0 + p0 + fk, ri = r0 + fr;
          const double xv = xcol[p * LD];
          const double a = ri > p ? xv : (ri == p ? dinv[b0 + h + p] : 0.0);
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, tb[p], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) L[(b0 + cc + ct * 16 + fr) * LD + b0 + h + r0 + fk + 4 * r] = -(acc[r] + acc2[r]);
      }
      __syncthreads();
      POTRF_STAMP();
    }
  }
  // inv = X (lower), invT = X' (upper): tile (ti, tj), tj <= ti, of inv and its mirror image (tj, ti) of invT
#pragma unroll
  for (int u = 0; u < 18; ++u) {
    int t0 = 2 * u, ti0 = 0;
    while ((ti0 + 1) * (ti0 + 2) / 2 <= t0) ++ti0;
    const int tj0 = t0 - ti0 * (ti0 + 1) / 2;
    int t1 = 2 * u + 1, ti1 = 0;
    while ((ti1 + 1) * (ti1 + 2) / 2 <= t1) ++ti1;
    const int tj1 = t1 - ti1 * (ti1 + 1) / 2;
    const int ti = th ? ti1 : ti0, tj = th ? tj1 : tj0;
    const int r = 16 * ti + tr, c = 16 * tj + tc;  // element (r, c) of inv, r >= c except above a diagonal tile's diagonal
    const double xl = L[c * LD + r];               // X(r, c) for r > c
    const int r2 = 16 * tj + tr, c2 = 16 * ti + tc;  // element (r2, c2) of invT, c2 >= r2 except below the diagonal
    const double xu = L[r2 * LD + c2];               // X(c2, r2) for c2 > r2
    if (ti != tj) {
      inv[(size_t)r * kDB + c] = xl;
      invT[(size_t)r2 * kDB + c2] = xu;
    } else {
      inv[(size_t)r * kDB + c] = c < r ? xl : (c == r ? dinv[r] : 0.0);
      invT[(size_t)r2 * kDB + c2] = c2 > r2 ? xu : (c2 == r2 ? dinv[r2] : 0.0);
    }
  }
  POTRF_STAMP();
}

// out[i][0] = sa * a[i], out[i][1] = sb * b[i] for i < len, zero on the padding
inline __global__ __launch_bounds__(256) void k_dense_pack2(const double* a, double sa, const double* b, double sb, double* out,
                                                     int len, int lenpad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= lenpad) return;
  out[(size_t)i * 2] = (i < len && a) ? sa * a[i] : 0.0;
  out[(size_t)i * 2 + 1] = (i < len && b) ? sb * b[i] : 0.0;
}

// out0[i] = in[i][0], out1[i] = in[i][1]
// the same with a row permutation: out{0,1}[perm[i]] = in[i][{0,1}]
inline __global__ __launch_bounds__(256) void k_unpack2_scatter(const double* __restrict__ in, const int32_t* __restrict__ perm,
                                                         double* out0, double* out1, int len) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= len) return;
  out0[perm[i]] = in[(size_t)i * 2];
  out1[perm[i]] = in[(size_t)i * 2 + 1];
}

inline __global__ __launch_bounds__(256) void k_dense_unpack2(const double* in, double* out0, double* out1, int len) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= len) return;
  out0[i] = in[(size_t)i * 2];
  out1[i] = in[(size_t)i * 2 + 1];
}

// Blocked triangular solves with the Cholesky factor (2 interleaved right-hand sides).
// forward step k:  y_k = Linv_kk r_k ;  r_i -= L_ik y_k (i > k).     backward step k:  q_k = Linv_kk' y_k ; y_i -= L_ki' q_k (i < k)
// One launch per step, one workgroup per 128-row block still to be updated plus one that stores the solved block.
// Every workgroup first recomputes the (tiny) diagonal solve of block k redundantly into LDS -- block k of `r` is
// only READ in this launch (the solved values go to `out`), so there is no race.
// The same step organised for LATENCY (the default): a step is a chain link of the triangular solve -- nb (dense) or
// 2 m / 128 (band) of them run back to back, each with a handful of workgroups -- so what counts is the number of
// dependent memory round trips inside it.  Here every global load of the step (the 128 x 128 inverse block AND the
// workgroup's own off-diagonal block, 64 + 64 values per thread) is issued before the first use: one round trip.  The
// triangular half of the inverse that is identically zero is skipped by whole waves.  Forward updates reduce their 64
// (row, right-hand side) partial products per wave with a transposing butterfly (63 shuffles instead of 384; lane l ends
// with the total of value l, stored coalesced); backward updates read the block by columns and need none.
template <bool FORWARD>
__global__ __launch_bounds__(256) void k_trsv_step3(const double* __restrict__ Lm, int ld, const double* __restrict__ inv,
                                                    const double* __restrict__ invT, double* r, double* out, int k,
                                                    int band_w = 0, int bstride = 1) {
  __shared__ double rk[kDB * 2];
  __shared__ double part[2][kDB * 2];
  __shared__ double yk[kDB * 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // (bstride = 2: the blocks of k's own elimination chain, fpsq_band_create)
  const int blk = FORWARD ? k + bstride * (int)blockIdx.x
                          : (band_w > 0 ? k - bstride * (int)blockIdx.x : (int)blockIdx.x);
  const int i = tid & 127, hf = tid >> 7;
  // forward: y_i = sum_{p <= i} X'[p][i] r_p;   backward: q_i = sum_{p >= i} X[p][i] y_p   (p in this thread's half)
  const double* Xc = (FORWARD ? invT : inv) + (size_t)k * kDB * kDB + (size_t)(hf * 64) * kDB + i;
  const bool xskip = FORWARD ? (hf == 1 && i < 64) : (hf == 0 && i >= 64);  // (wave-uniform) all-zero part of the triangle
  double xs[64], lb[64];
  if (!xskip) {
#pragma unroll
    for (int q = 0; q < 64; ++q) xs[q] = Xc[(size_t)q * kDB];
  }
  const size_t lds = band_w > 0 ? (size_t)kDB : (size_t)ld;
  if (blk != k) {
    if (FORWARD) {  // block (blk, k), rows 32 wave .. + 31, lanes along the columns
      const double* Lb = (band_w > 0 ? Lm + ((size_t)blk * band_w + (k - blk + band_w - 1)) * kDB * kDB
                                     : Lm + (size_t)(blk * kDB) * ld + k * kDB) + (size_t)(wave * 32) * lds + lane;
#pragma unroll
      for (int u = 0; u < 32; ++u) {
        lb[2 * u] = Lb[(size_t)u * lds];
        lb[2 * u + 1] = Lb[(size_t)u * lds + 64];
      }
    } else {  // block (k, blk) read by columns: column i, rows of this thread's half
      const double* Lb = (band_w > 0 ? Lm + ((size_t)k * band_w + (blk - k + band_w - 1)) * kDB * kDB
                                     : Lm + (size_t)(k * kDB) * ld + blk * kDB) + (size_t)(hf * 64) * lds + i;
#pragma unroll
      for (int q = 0; q < 64; ++q) lb[q] = Lb[(size_t)q * lds];
    }
  }
  rk[tid] = r[(size_t)(k * kDB) * 2 + tid];
  __syncthreads();
  {
    double s0 = 0.0, s1 = 0.0;
    if (!xskip) {
#pragma unroll
      for (int q = 0; q < 64; ++q) {
        s0 += xs[q] * rk[(hf * 64 + q) * 2];
        s1 += xs[q] * rk[(hf * 64 + q) * 2 + 1];
      }
    }
    part[hf][i * 2] = s0;
    part[hf][i * 2 + 1] = s1;
  }
  __syncthreads();
  yk[tid] = part[0][tid] + part[1][tid];
  __syncthreads();
  if (blk == k) {
    out[(size_t)(k * kDB) * 2 + tid] = yk[tid];
    return;
  }
  if (FORWARD) {
    const double y00 = yk[lane * 2], y01 = yk[lane * 2 + 1], y10 = yk[(lane + 64) * 2], y11 = yk[(lane + 64) * 2 + 1];
    double v[64];
#pragma unroll
    for (int u = 0; u < 32; ++u) {
      v[2 * u] = lb[2 * u] * y00 + lb[2 * u + 1] * y10;
      v[2 * u + 1] = lb[2 * u] * y01 + lb[2 * u + 1] * y11;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const bool hi = (lane & off) != 0;
#pragma unroll
      for (int idx = 0; idx < off; ++idx) {
        const double send = hi ? v[idx] : v[idx + off];
        const double keep = hi ? v[idx + off] : v[idx];
        v[idx] = keep + __shfl_xor(send, off, 64);
      }
    }
    r[(size_t)(blk * kDB + wave * 32) * 2 + lane] -= v[0];
  } else {
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int q = 0; q < 64; ++q) {
      s0 += lb[q] * yk[(hf * 64 + q) * 2];
      s1 += lb[q] * yk[(hf * 64 + q) * 2 + 1];
    }
    __syncthreads();
    part[hf][i * 2] = s0;
    part[hf][i * 2 + 1] = s1;
    __syncthreads();
    r[(size_t)(blk * kDB) * 2 + tid] -= part[0][tid] + part[1][tid];
  }
}

// ---- the whole sweep in ONE launch (the default; FPSQ_TRSV_CHAIN=0 selects the step kernels above).  A sweep is a chain of
// nb links and a launch per link costs ~3.5 us of dispatch before its single memory round trip starts (8.5 / 6.3 us per
// forward / backward step).  Here workgroup w owns block b (forward: b = w, backward: b = nb - 1 - w) and PULLS: for every
// coupled block j eliminated before b it takes the solved y_j from the publication buffer, subtracts L_bj y_j (forward) or
// L_jb' q_j (backward) from its own right-hand side -- kept in registers, thread t <-> entry t of the [128][2] block --, then
// solves with the diagonal inverse and publishes.  Publication as in the product kernels' leader records (fpsq_spmv.hip.h):
// every 8-byte word carries half a double and the launch number `seq`, written through and read with agent-scope atomics,
// so a reader that sees the number sees the payload: no flag, no fence, one round trip per look, and the look IS the
// fetch.  WHICH block a workgroup owns is decided by a TICKET it draws when it starts (one agent-scope atomic add; round 4),
// not by its index in the grid: dependencies point to lower tickets only, and a lower ticket is held by a workgroup that
// is already RUNNING -- whatever else shares the device.  (By grid index -- round 3 -- that only holds inside one kernel:
// workgroup i is dispatched by XCD i mod 8, in order within that XCD, so with a second sweep on the device -- another
// handle, stream or process -- XCD a can be full of kernel Y's waiting workgroups while X's lowest unfinished block is not
// yet dispatched there, and vice versa: the circular wait across kernels that the riding leaders of the product kernels
// ran into, fpsq_spmv.hip.h "WHO LEADS".  The ticket's round trip, ~1.5 us, is paid once per workgroup at its start, long
// before its turn in a 50-70 us sweep.)  Every wait is bounded all the same (kChainPolls looks, then the error word is
// raised and the workgroup goes on publishing, so nobody behind it waits in turn; an abort word behind the buffer, set with
// it and looked at before and during every wait, keeps the waits that are still to come short: a failed sweep ends after ONE
// waiting time, not one per link; the call fails with FPSQ_ERR_TIMEOUT).
// coupled(b, j) for the banded factor with two elimination chains (fpsq_band_create): inside the chain region (both < 2 cs)
// only blocks of the same parity within 2 cb; otherwise the plain band |b - j| <= w.  Dense: w = nb, cs = 0.
// The off-diagonal block of a link is requested BEFORE the look at y_j: it is in flight while the workgroup waits.
constexpr int kChainPolls = 1 << 20;
struct ChainArgs {
  unsigned long long* pub;  // [nb][512]: block j's 256 doubles as (high half | seq), (low half << 32 | seq); [nb * 512]: abort
  unsigned int seq;
  unsigned int pubseq;      // what a workgroup publishes: `seq` (anything else only in the test of the bounded wait)
  int nb, band_w, cs, cb;
  unsigned long long* err;  // host-mapped
  unsigned long long* ticket;      // monotone counter (never reset): this launch's workgroups draw ticket_base .. + nb - 1
  unsigned long long ticket_base;
};
__device__ __forceinline__ bool chain_coupled(const ChainArgs& c, int b, int j) {
  const int w = c.band_w > 0 ? c.band_w - 1 : c.nb;
  const int d = b > j ? b - j : j - b;
  if (b < 2 * c.cs && j < 2 * c.cs) return (d & 1) == 0 && d <= 2 * c.cb;
  return d <= w;
}
// this thread's entry of block j's published vector (bounded wait)
__device__ __forceinline__ double chain_take(const ChainArgs& c, int j) {
  const unsigned long long* p = c.pub + (size_t)j * 512 + 2 * threadIdx.x;
  unsigned long long* ab = c.pub + (size_t)c.nb * 512;
  unsigned long long w0, w1;
  int n = __hip_atomic_load(ab, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == c.seq ? kChainPolls : 0;
  for (;;) {
    w0 = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    w1 = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (((unsigned int)w0 == c.seq && (unsigned int)w1 == c.seq) || ++n >= kChainPolls) break;
    if ((n & 1023) == 0 && __hip_atomic_load(ab, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == c.seq) n = kChainPolls - 1;
    __builtin_amdgcn_s_sleep(2);
  }
  if (n >= kChainPolls) {
    __hip_atomic_store(ab, (unsigned long long)c.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(c.err, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  return __longlong_as_double((long long)((w0 & 0xffffffff00000000ull) | (w1 >> 32)));
}
template <bool FORWARD>
__global__ __launch_bounds__(256) void k_trsv_chain(const double* __restrict__ Lm, int ld, const double* __restrict__ inv,
                                                    const double* __restrict__ invT, const double* __restrict__ r, double* out,
                                                    ChainArgs c) {
  __shared__ double rk[kDB * 2];
  __shared__ double part[2][kDB * 2];
  __shared__ double yk[kDB * 2];
  __shared__ int ticket;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0)
    ticket = (int)(__hip_atomic_fetch_add(c.ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - c.ticket_base);
  __syncthreads();
  const int b = FORWARD ? ticket : c.nb - 1 - ticket;
  const int i = tid & 127, hf = tid >> 7;
  const double* Xc = (FORWARD ? invT : inv) + (size_t)b * kDB * kDB + (size_t)(hf * 64) * kDB + i;
  const bool xskip = FORWARD ? (hf == 1 && i < 64) : (hf == 0 && i >= 64);  // (wave-uniform) all-zero part of the triangle
  double xs[64];
  if (!xskip) {
#pragma unroll
    for (int q = 0; q < 64; ++q) xs[q] = Xc[(size_t)q * kDB];
  }
  double racc = r[(size_t)b * (kDB * 2) + tid];
  const int band_w = c.band_w;
  const size_t lds = band_w > 0 ? (size_t)kDB : (size_t)ld;
  const int w = band_w > 0 ? band_w - 1 : c.nb;
  if (FORWARD) {
    for (int j = max(0, b - w); j < b; ++j) {
      if (!chain_coupled(c, b, j)) continue;
      // block (b, j), rows 32 wave .. + 31, lanes along the columns
      const double* Lb = (band_w > 0 ? Lm + ((size_t)b * band_w + (j - b + band_w - 1)) * kDB * kDB
                                     : Lm + (size_t)(b * kDB) * ld + j * kDB) + (size_t)(wave * 32) * lds + lane;
      double lb[64];
#pragma unroll
      for (int u = 0; u < 32; ++u) {
        lb[2 * u] = Lb[(size_t)u * lds];
        lb[2 * u + 1] = Lb[(size_t)u * lds + 64];
      }
      yk[tid] = chain_take(c, j);
      __syncthreads();
      const double y00 = yk[lane * 2], y01 = yk[lane * 2 + 1], y10 = yk[(lane + 64) * 2], y11 = yk[(lane + 64) * 2 + 1];
      double v[64];
#pragma unroll
      for (int u = 0; u < 32; ++u) {
        v[2 * u] = lb[2 * u] * y00 + lb[2 * u + 1] * y10;
        v[2 * u + 1] = lb[2 * u] * y01 + lb[2 * u + 1] * y11;
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const bool hi = (lane & off) != 0;
#pragma unroll
        for (int idx = 0; idx < off; ++idx) {
          const double send = hi ? v[idx] : v[idx + off];
          const double keep = hi ? v[idx + off] : v[idx];
          v[idx] = keep + __shfl_xor(send, off, 64);
        }
      }
      racc -= v[0];
      __syncthreads();  // (yk is overwritten by the next link)
    }
  } else {
    for (int j = min(c.nb - 1, b + w); j > b; --j) {
      if (!chain_coupled(c, b, j)) continue;
      // block (j, b) read by columns: column i, rows of this thread's half
      const double* Lb = (band_w > 0 ? Lm + ((size_t)j * band_w + (b - j + band_w - 1)) * kDB * kDB
                                     : Lm + (size_t)(j * kDB) * ld + b * kDB) + (size_t)(hf * 64) * lds + i;
      double lb[64];
#pragma unroll
      for (int q = 0; q < 64; ++q) lb[q] = Lb[(size_t)q * lds];
      yk[tid] = chain_take(c, j);
      __syncthreads();
      double s0 = 0.0, s1 = 0.0;
#pragma unroll
      for (int q = 0; q < 64; ++q) {
        s0 += lb[q] * yk[(hf * 64 + q) * 2];
        s1 += lb[q] * yk[(hf * 64 + q) * 2 + 1];
      }
      part[hf][i * 2] = s0;
      part[hf][i * 2 + 1] = s1;
      __syncthreads();
      racc -= part[0][tid] + part[1][tid];
      __syncthreads();  // (part and yk are overwritten by the next link)
    }
  }
  // forward: y_i = sum_{p <= i} X'[p][i] r_p;   backward: q_i = sum_{p >= i} X[p][i] y_p   (p in this thread's half)
  rk[tid] = racc;
  __syncthreads();
  {
    double s0 = 0.0, s1 = 0.0;
    if (!xskip) {
#pragma unroll
      for (int q = 0; q < 64; ++q) {
        s0 += xs[q] * rk[(hf * 64 + q) * 2];
        s1 += xs[q] * rk[(hf * 64 + q) * 2 + 1];
      }
    }
    part[hf][i * 2] = s0;
    part[hf][i * 2 + 1] = s1;
  }
  __syncthreads();
  const double y = part[0][tid] + part[1][tid];
  const unsigned long long bits = (unsigned long long)__double_as_longlong(y);
  unsigned long long* p = c.pub + (size_t)b * 512 + 2 * tid;
  __hip_atomic_store(p, (bits & 0xffffffff00000000ull) | c.pubseq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(p + 1, (bits << 32) | c.pubseq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  out[(size_t)b * (kDB * 2) + tid] = y;
}

// ---- the same chained sweep for a TILE of 16 right-hand-side columns (8 vectors x the two M-solves) on the banded factor,
// on the fp64 matrix cores (fpsq_band_*_block).  A sweep of k_trsv_chain streams the whole factor for two columns; every
// further column carried through the serial chain and the stream costs no byte of the factor.  The protocol is
// k_trsv_chain's, unchanged: one launch per sweep, the block by ticket, chain_coupled for the band and the two chains, the
// off-diagonal block requested before the look at Y_j, publication words that carry half a double and the launch number,
// bounded waits that end in the error word and shorten behind the abort word.  What differs is the arithmetic of a link,
// R_b -= L_bj Y_j with Y_j 128 x 16: 8 x 32 v_mfma_f64_16x16x4_f64, 64 per wave, each wave 32 rows of the block.
// The summation index of an MFMA is free, and so is which 16 rows form a tile; both are chosen so that a lane's global
// loads are 16 bytes wide and the fragments need no LDS:
//   rows of wave T, tile e (0 / 1), lane l = (i = l & 15, g = l >> 4):  row(e, i) = 32 T + 2 i + e   (interleaved pairs);
//   D register r of tile e is row 32 T + 2 (g + 4 r) + e, column i -- the layout of the right-hand side in registers, of a
//   thread's 8 publication slots and of its 8 stores, the same in both sweeps;
//   "by columns" (backward links, both diagonal solves: A[i][k] = X[k][row]): step s takes k = 4 s + g, one 16-byte load
//   X[k][32 T + 2 i .. + 1] feeds both tiles -- 16 lanes read 256 contiguous bytes;
//   "by rows" (forward links: A[i][k] = L[row][k]): chunk c of 8 columns, lane group g takes k = 8 c + 2 g + h (h = 0 / 1) from
//   one 16-byte load per tile -- 4 lane groups read 64 contiguous bytes of each of 16 rows.
// Y_j / the right-hand side for the diagonal solve go through LDS as [128][16] (a B fragment is 16 consecutive doubles per
// lane group: conflict-free).  Every column of D is summed in the same fixed order whatever the other columns hold, so a
// column's result does not depend on its position, on the other columns or on how many there are (short tiles are padded
// with zero columns by the product kernels).  Even and odd steps accumulate separately (two dependent MFMA chains per
// tile instead of one) and are added at the end of a link.  The diagonal solve skips the steps that lie wholly in the zero
// triangle of the inverse (wave-uniform).
// pub: [nb][4096] words -- slot q of thread t of block j at (q * 256 + t) * 2 --, [nb * 4096]: abort, [nb * 4096 + 1]: tickets.
constexpr int kBlkCols = 16;                 // right-hand-side columns of a tile
constexpr int kBlkPub = kDB * kBlkCols * 2;  // publication words of a block
// this thread's 8 entries of block j's published tile, written to LDS in the [128][16] layout (bounded wait)
__device__ __forceinline__ void chain_take16(const ChainArgs& c, int j, double* __restrict__ ylds, int row0, int col) {
  const unsigned long long* p = c.pub + (size_t)j * kBlkPub + 2 * threadIdx.x;
  unsigned long long* ab = c.pub + (size_t)c.nb * kBlkPub;
  unsigned long long w[16];
  int n = __hip_atomic_load(ab, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == c.seq ? kChainPolls : 0;
  for (;;) {
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      w[2 * q] = __hip_atomic_load(p + q * 512, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      w[2 * q + 1] = __hip_atomic_load(p + q * 512 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) ok = ok && (unsigned int)w[q] == c.seq;
    if (ok || ++n >= kChainPolls) break;
    if ((n & 1023) == 0 && __hip_atomic_load(ab, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == c.seq) n = kChainPolls - 1;
    __builtin_amdgcn_s_sleep(2);
  }
  if (n >= kChainPolls) {
    __hip_atomic_store(ab, (unsigned long long)c.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(c.err, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
#pragma unroll
  for (int q = 0; q < 8; ++q)  // slot q = tile q >> 2, register q & 3
    ylds[(row0 + 8 * (q & 3) + (q >> 2)) * kBlkCols + col] =
        __longlong_as_double((long long)((w[2 * q] & 0xffffffff00000000ull) | (w[2 * q + 1] >> 32)));
}
// P[e] = sum over the steps s0 <= s < s1 of the "by columns" product (xs[s] = X[4 s + g][row(0, i) .. + 1]) with the tile in ylds
__device__ __forceinline__ void blk_mma_cols(const f64x2 (&xs)[32], const double* __restrict__ ylds, int g, int i, int s0,
                                             int s1, f64x4 (&P)[2]) {
  f64x4 a0[2] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}}, a1[2] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
#pragma unroll
  for (int s = 0; s < 32; ++s) {
    if (s >= s0 && s < s1) {  // (wave-uniform)
      const double y = ylds[(4 * s + g) * kBlkCols + i];
      a0[s & 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(xs[s][0], y, a0[s & 1], 0, 0, 0);
      a1[s & 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(xs[s][1], y, a1[s & 1], 0, 0, 0);
    }
  }
  P[0] = a0[0] + a0[1];
  P[1] = a1[0] + a1[1];
}
template <bool FORWARD>
__global__ __launch_bounds__(256) void k_trsm_chain16(const double* __restrict__ Lm, const double* __restrict__ inv,
                                                      const double* __restrict__ invT, const double* __restrict__ r,
                                                      double* out, ChainArgs c) {
  __shared__ double yk[kDB * kBlkCols];
  __shared__ int ticket;
  const int tid = threadIdx.x, lane = tid & 63, T = tid >> 6;
  const int fi = lane & 15, fg = lane >> 4;
  if (tid == 0)
    ticket = (int)(__hip_atomic_fetch_add(c.ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - c.ticket_base);
  __syncthreads();
  const int b = FORWARD ? ticket : c.nb - 1 - ticket;
  const int row0 = 32 * T + 2 * fg;  // row of register r of tile e: row0 + 8 r + e
  // forward: Y = inv R = sum_k invT[k][row] R[k], k <= row;   backward: Q = inv' Y = sum_k inv[k][row] Y[k], k >= row
  const int s0 = FORWARD ? 0 : 8 * T, s1 = FORWARD ? 8 * (T + 1) : 32;
  f64x2 xs[32];
  {
    const double* Xc = (FORWARD ? invT : inv) + (size_t)b * kDB * kDB + (size_t)fg * kDB + 32 * T + 2 * fi;
#pragma unroll
    for (int s = 0; s < 32; ++s)
      if (s >= s0 && s < s1) xs[s] = *reinterpret_cast<const f64x2*>(Xc + (size_t)(4 * s) * kDB);
  }
  f64x4 racc[2];
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int q = 0; q < 4; ++q) racc[e][q] = r[((size_t)b * kDB + row0 + 8 * q + e) * kBlkCols + fi];
  const int band_w = c.band_w, w = band_w - 1;
  if (FORWARD) {
    for (int j = max(0, b - w); j < b; ++j) {
      if (!chain_coupled(c, b, j)) continue;
      // block (b, j) by rows: lb[e][cc] = L[32 T + 2 fi + e][8 cc + 2 fg .. + 1]
      const double* Lb = Lm + ((size_t)b * band_w + (j - b + band_w - 1)) * kDB * kDB + (size_t)(32 * T + 2 * fi) * kDB + 2 * fg;
      f64x2 lb[2][16];
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) {
        lb[0][cc] = *reinterpret_cast<const f64x2*>(Lb + 8 * cc);
        lb[1][cc] = *reinterpret_cast<const f64x2*>(Lb + kDB + 8 * cc);
      }
      chain_take16(c, j, yk, row0, fi);
      __syncthreads();
      f64x4 a0[2] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}}, a1[2] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
#pragma unroll
      for (int cc = 0; cc < 16; ++cc)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const double y = yk[(8 * cc + 2 * fg + h) * kBlkCols + fi];
          a0[h] = __builtin_amdgcn_mfma_f64_16x16x4f64(lb[0][cc][h], y, a0[h], 0, 0, 0);
          a1[h] = __builtin_amdgcn_mfma_f64_16x16x4f64(lb[1][cc][h], y, a1[h], 0, 0, 0);
        }
      racc[0] -= a0[0] + a0[1];
      racc[1] -= a1[0] + a1[1];
      __syncthreads();  // (yk is overwritten by the next link)
    }
  } else {
    for (int j = min(c.nb - 1, b + w); j > b; --j) {
      if (!chain_coupled(c, b, j)) continue;
      // block (j, b) by columns: lb[s] = L[4 s + fg][32 T + 2 fi .. + 1]
      const double* Lb = Lm + ((size_t)j * band_w + (b - j + band_w - 1)) * kDB * kDB + (size_t)fg * kDB + 32 * T + 2 * fi;
      f64x2 lb[32];
#pragma unroll
      for (int s = 0; s < 32; ++s) lb[s] = *reinterpret_cast<const f64x2*>(Lb + (size_t)(4 * s) * kDB);
      chain_take16(c, j, yk, row0, fi);
      __syncthreads();
      f64x4 P[2];
      blk_mma_cols(lb, yk, fg, fi, 0, 32, P);
      racc[0] -= P[0];
      racc[1] -= P[1];
      __syncthreads();  // (yk is overwritten by the next link)
    }
  }
  // the diagonal solve: the right-hand side through LDS as the B operand
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int q = 0; q < 4; ++q) yk[(row0 + 8 * q + e) * kBlkCols + fi] = racc[e][q];
  __syncthreads();
  f64x4 Y[2];
  blk_mma_cols(xs, yk, fg, fi, s0, s1, Y);
  unsigned long long* p = c.pub + (size_t)b * kBlkPub + 2 * tid;
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned long long bits = (unsigned long long)__double_as_longlong(Y[e][q]);
      __hip_atomic_store(p + (4 * e + q) * 512, (bits & 0xffffffff00000000ull) | c.pubseq, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(p + (4 * e + q) * 512 + 1, (bits << 32) | c.pubseq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int q = 0; q < 4; ++q) out[((size_t)b * kDB + row0 + 8 * q + e) * kBlkCols + fi] = Y[e][q];
}

// jac_coord! hand-over on the device (src/solve_linear_system.jl:223-233: `jac_coord!` then `sparse(rows, cols, vals)`):
// slot i of the back-end's own storage = the sum of the caller's COO entries perm[slotptr[i] .. slotptr[i + 1]) in that
// (sorted, fixed) order -- duplicates are summed like SparseArrays.sparse does, deterministically; slotptr == null: one
// entry per slot.  target != null: the slot lives at out[target[i]] (dense row-major storage), else at out[i].
inline __global__ __launch_bounds__(256) void k_coo_to_slots(const double* __restrict__ coo, const int32_t* __restrict__ perm,
                                                      const int32_t* __restrict__ slotptr, const int64_t* __restrict__ target,
                                                      double* __restrict__ out, int64_t nslots) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nslots; i += (int64_t)gridDim.x * 256) {
    double v;
    if (slotptr) {
      v = 0.0;
      for (int k = slotptr[i]; k < slotptr[i + 1]; ++k) v += coo[perm[k]];
    } else {
      v = coo[perm[i]];
    }
    out[target ? target[i] : i] = v;
  }
}

}  // namespace fpsq

// ===================================================================== host scaffold of the two direct back-ends

namespace fpsq_direct {
using namespace fpsq;

// What the dense and the banded direct handle share: everything around their numeric cores (storage and formation of M, the
// elimination order).  Each handle derives from it and adds only its own storage.
struct DirectCore {
  const char* name = "";  // "dense" / "band": prefix of the state errors
  int64_t n = 0, m = 0, mpad = 0, nb = 0;
  int64_t vrows = 0;  // slots behind row mpad of r2 / r16 that no sweep touches (fpsq_band: the long columns' virtual rows)
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  bool factored = false;
  double* invs = nullptr;   // nb inverses of the diagonal 128 x 128 blocks of L
  double* invsT = nullptr;  // ... and their transposes (k_potrf_inv128m, k_trsv_step3)
  double *r2 = nullptr, *y2 = nullptr;  // [mpad][2] each: right-hand sides / solutions of the two M-solves
  double *in_a = nullptr, *in_b = nullptr, *o_p1 = nullptr, *o_p2 = nullptr, *o_q1 = nullptr, *o_q2 = nullptr;
  int* info_dev = nullptr;
  double piv_tol = 0.0, piv_reg = 0.0;  // dynamic regularisation (fpsq_*_set_regularization); reg <= 0: off
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
  // the triangular sweeps in one launch each (k_trsv_chain): publication buffer, launch number, host-mapped error word
  unsigned long long* chain_pub = nullptr;
  unsigned long long* chain_err = nullptr;
  unsigned int chain_seq = 0;
  bool chain = true;         // FPSQ_TRSV_CHAIN=0: one launch per step (k_trsv_step3)
  bool chain_break = false;  // FPSQ_DEBUG_CHAIN_BREAK=1 (tests): the workgroups publish a wrong launch number
  // jac_coord! hand-over: the caller's COO entries sorted into slots (entries of A / of the CSR), duplicates grouped
  int64_t coo_nnz = -1;
  int32_t *coo_perm = nullptr, *coo_slotptr = nullptr;
  double* coo_in = nullptr;
  // device-resident evaluations (fpsq_band_qp_*): the caller's producer stream (include/fpsq.h "INPUT READINESS") and the
  // scalars of a call, device side and pinned host side
  bool in_stream_on = false;
  hipStream_t in_stream = nullptr;
  hipEvent_t ev_in = nullptr;
  double *scal = nullptr, *scal_host = nullptr;
  // the sweeps over a tile of 16 right-hand-side columns (k_trsm_chain16), allocated by the first block call: right-hand
  // sides / solutions [mpad][16], publication buffer [nb][4096] + abort word + ticket word, launch number
  double *r16 = nullptr, *y16 = nullptr;
  unsigned long long* blk_pub = nullptr;
  unsigned int blk_seq = 0;
  std::vector<void*> allocs;
};

// COO triplets (any order, duplicates allowed, `base`-based) -> row-major sorted slots.  order[k]: the caller's index of the
// k-th sorted entry (stable: duplicates keep the caller's order); slotptr: one range of sorted entries per distinct (row,
// col); srow / scol: the slots' coordinates.  Returns an error text, empty on success.
inline std::string coo_sort(int64_t m, int64_t n, int64_t nnz, const int64_t* rows, const int64_t* cols, int32_t base,
                            std::vector<int32_t>& order, std::vector<int32_t>& slotptr, std::vector<int32_t>& srow,
                            std::vector<int32_t>& scol) {
  std::vector<int32_t> cnt(m + 1, 0);
  for (int64_t k = 0; k < nnz; ++k) {
    const int64_t r = rows[k] - base, c = cols[k] - base;
    if (r < 0 || r >= m || c < 0 || c >= n) return "COO index out of range";
    cnt[r + 1]++;
  }
  for (int64_t i = 0; i < m; ++i) cnt[i + 1] += cnt[i];
  order.resize(nnz);
  {
    std::vector<int32_t> next(cnt.begin(), cnt.end() - 1);
    for (int64_t k = 0; k < nnz; ++k) order[next[rows[k] - base]++] = (int32_t)k;
  }
  for (int64_t i = 0; i < m; ++i)
    std::stable_sort(order.begin() + cnt[i], order.begin() + cnt[i + 1],
                     [&](int32_t a, int32_t b) { return cols[a] < cols[b]; });
  slotptr.assign(1, 0);
  srow.clear();
  scol.clear();
  for (int64_t i = 0; i < m; ++i)
    for (int32_t k = cnt[i]; k < cnt[i + 1]; ++k) {
      const int64_t c = cols[order[k]] - base;
      if (k > cnt[i] && c == cols[order[k - 1]] - base) {
        slotptr.back() = k + 1;
      } else {
        srow.push_back((int32_t)i);
        scol.push_back((int32_t)c);
        slotptr.push_back(k + 1);
      }
    }
  return "";
}

#define CHK(c, call)                                                           \
  do {                                                                         \
    hipError_t e_ = (call);                                                    \
    if (e_ != hipSuccess) {                                                    \
      (c)->err = std::string(#call) + ": " + hipGetErrorString(e_);            \
      return FPSQ_ERR_HIP;                                                     \
    }                                                                          \
  } while (0)

template <class T>
int dalloc(DirectCore* c, T** p, size_t count) {
  void* q = nullptr;
  CHK(c, hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)));
  c->allocs.push_back(q);
  *p = (T*)q;
  return 0;
}

// grid of a kernel that gives one thread of its 256-thread workgroups to each of `len` elements
inline dim3 grid256(int64_t len) { return dim3((unsigned)((len + 255) / 256)); }

// Set-up of the shared part on the handle's device (n, m, mpad, nb and the stream are the create function's: it owns the
// error texts): events, the buffers every solve uses (`nlen`: the stored length of an n-vector), the chain publication
// buffer, the host-mapped error word, the two environment switches.  Non-zero: failed, c->err says why.
inline int core_setup(DirectCore* c, int64_t nlen) {
  hipEventCreate(&c->e0);
  hipEventCreate(&c->e1);
  hipEventCreate(&c->e2);
  const size_t inv_len = (size_t)c->nb * kDB * kDB;
  int rc = dalloc(c, &c->invs, inv_len) | dalloc(c, &c->invsT, inv_len);
  if (!rc) {  // k_potrf_inv128m writes the non-zero triangles only
    hipMemset(c->invs, 0, inv_len * 8);
    hipMemset(c->invsT, 0, inv_len * 8);
  }
  rc |= dalloc(c, &c->r2, (size_t)(c->mpad + c->vrows) * 2) | dalloc(c, &c->y2, (size_t)c->mpad * 2);
  rc |= dalloc(c, &c->in_a, (size_t)nlen) | dalloc(c, &c->in_b, (size_t)std::max(nlen, c->mpad));
  rc |= dalloc(c, &c->o_p1, (size_t)nlen) | dalloc(c, &c->o_p2, (size_t)nlen);
  rc |= dalloc(c, &c->o_q1, (size_t)c->mpad) | dalloc(c, &c->o_q2, (size_t)c->mpad) | dalloc(c, &c->info_dev, 4);
  const size_t pub_len = (size_t)c->nb * 512 + 8;  // (+ the abort word)
  rc |= dalloc(c, &c->chain_pub, pub_len);
  if (!rc) hipMemset(c->chain_pub, 0, pub_len * 8);
  if (hipHostMalloc((void**)&c->chain_err, 8, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) rc = 1;
  else *c->chain_err = 0;
  if (const char* e = getenv("FPSQ_TRSV_CHAIN")) c->chain = atoi(e) != 0;
  if (const char* e = getenv("FPSQ_DEBUG_CHAIN_BREAK")) c->chain_break = atoi(e) != 0;
  return rc;
}

// ... and its tear-down, the stream included; the handle itself is the caller's to delete
inline void core_teardown(DirectCore* c) {
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  for (void* p : c->allocs) hipFree(p);
  if (c->chain_err) hipHostFree(c->chain_err);
  if (c->scal_host) hipHostFree(c->scal_host);
  if (c->ev_in) hipEventDestroy(c->ev_in);
  if (c->e0) hipEventDestroy(c->e0);
  if (c->e1) hipEventDestroy(c->e1);
  if (c->e2) hipEventDestroy(c->e2);
  if (c->stream) hipStreamDestroy(c->stream);
}

inline int set_regularization(DirectCore* c, double tol, double reg) {
  if (!c || !(tol >= 0.0)) return FPSQ_ERR_ARG;
  c->piv_tol = tol;
  c->piv_reg = reg;
  return FPSQ_OK;
}

// jac_coord! hand-over: the caller's values (host or device) into `nslots` sorted slots of `out` (at target[slot] when given),
// duplicates summed in the caller's order; left in flight on c->stream
inline int coo_to_slots(DirectCore* c, const double* vals, const int64_t* target, double* out, int64_t nslots) {
  CHK(c, hipMemcpyAsync(c->coo_in, vals, (size_t)c->coo_nnz * 8, hipMemcpyDefault, c->stream));
  hipLaunchKernelGGL(k_coo_to_slots, dim3((unsigned)std::min<int64_t>((nslots + 255) / 256, 4096)), dim3(256), 0, c->stream,
                     c->coo_in, c->coo_perm, c->coo_slotptr, target, out, nslots);
  return FPSQ_OK;
}

// potrf + inverse of diagonal block k (at Mkk, leading dimension ld) on stream q; returns the inverse
#ifndef FPSQ_POTRF_TIMING  // (tools/potrf_probe.hip launches the kernel itself, with one more argument)
inline double* launch_potrf(DirectCore* c, hipStream_t q, double* Mkk, int ld, int k) {
  double* inv = c->invs + (size_t)k * kDB * kDB;
  hipLaunchKernelGGL(k_potrf_inv128m, dim3(1), dim3(kPotrfThreads5), kPotrfLds5, q, Mkk, ld, inv,
                     c->invsT + (size_t)k * kDB * kDB, k * kDB, c->info_dev, c->piv_tol, c->piv_reg);
  return inv;
}
#endif

// End of a factorisation whose caller recorded e0 (start) and e1 (M formed) on c->stream: device times, regularised pivots,
// `factored`.  *pivot: first non-positive pivot row (1-based, stored numbering; 0: none).  Returns 1 (soft) when there is
// one: M not positive definite (the reference warns and goes on, src/solve_linear_system.jl:242-246).
inline int factor_end(DirectCore* c, double* form_ms, double* chol_ms, int64_t* regularized, int32_t* pivot) {
  hipEventRecord(c->e2, c->stream);
  int32_t hinfo[2] = {0, 0};
  CHK(c, hipMemcpyAsync(hinfo, c->info_dev, 8, hipMemcpyDeviceToHost, c->stream));
  CHK(c, hipStreamSynchronize(c->stream));
  float a = 0.f, b = 0.f;
  hipEventElapsedTime(&a, c->e0, c->e1);
  hipEventElapsedTime(&b, c->e1, c->e2);
  *form_ms = a;
  *chol_ms = b;
  *regularized = hinfo[1];
  *pivot = hinfo[0];
  c->factored = hinfo[0] == 0;
  return hinfo[0] == 0 ? FPSQ_OK : 1;
}

// The two triangular sweeps in one launch each, forward then backward, publishing through `pub` (`words` per block, behind
// them the abort word and the ticket word: it counts every workgroup of every sweep that uses this buffer, nb per launch);
// `seq` numbers the buffer's launches.  band_w / chain_safe / chain_bw: the band geometry, 0 / 0 / 0 for a full lower triangle.
template <class Fwd, class Bwd>
void chain_launches(DirectCore* c, unsigned long long* pub, size_t words, unsigned int& seq, int band_w, int chain_safe,
                    int chain_bw, Fwd forward, Bwd backward) {
  const int nb = (int)c->nb;
  ChainArgs a{pub, 0, 0, nb, band_w, chain_safe, chain_bw, c->chain_err, pub + (size_t)nb * words + 1, 0};
  auto next = [&] {
    a.seq = ++seq;
    a.pubseq = c->chain_break ? ~a.seq : a.seq;
    a.ticket_base = (unsigned long long)(seq - 1) * nb;
  };
  next();
  forward(a);
  next();
  backward(a);
}

// c->r2 <- M^-1 c->r2 via L y = r (into c->y2), L' q = y, with the factor at M (leading dimension ld)
inline void chain_sweeps(DirectCore* c, const double* M, int ld, int band_w, int chain_safe, int chain_bw) {
  const dim3 nb((unsigned)c->nb);
  auto fwd = [&](const ChainArgs& a) {
    hipLaunchKernelGGL(k_trsv_chain<true>, nb, dim3(256), 0, c->stream, M, ld, c->invs, c->invsT, c->r2, c->y2, a);
  };
  auto bwd = [&](const ChainArgs& a) {
    hipLaunchKernelGGL(k_trsv_chain<false>, nb, dim3(256), 0, c->stream, M, ld, c->invs, c->invsT, c->y2, c->r2, a);
  };
  chain_launches(c, c->chain_pub, 512, c->chain_seq, band_w, chain_safe, chain_bw, fwd, bwd);
}

// The same for a tile of 16 columns on the banded factor: c->r16 <- M^-1 c->r16 (via c->y16), with a publication buffer and
// a launch number of its own.  chain16_setup allocates the buffers at the first call (they are freed with the handle);
// non-zero: failed.
inline int chain16_setup(DirectCore* c) {
  if (c->blk_pub) return FPSQ_OK;
  const size_t pub_len = (size_t)c->nb * kBlkPub + 8;
  unsigned long long* pub = nullptr;
  if (dalloc(c, &c->r16, (size_t)(c->mpad + c->vrows) * kBlkCols) || dalloc(c, &c->y16, (size_t)c->mpad * kBlkCols) ||
      dalloc(c, &pub, pub_len))
    return FPSQ_ERR_HIP;
  CHK(c, hipMemsetAsync(pub, 0, pub_len * 8, c->stream));
  c->blk_pub = pub;
  return FPSQ_OK;
}

inline void chain_sweeps16(DirectCore* c, const double* Mb, int band_w, int chain_safe, int chain_bw) {
  const dim3 nb((unsigned)c->nb);
  auto fwd = [&](const ChainArgs& a) {
    hipLaunchKernelGGL(k_trsm_chain16<true>, nb, dim3(256), 0, c->stream, Mb, c->invs, c->invsT, c->r16, c->y16, a);
  };
  auto bwd = [&](const ChainArgs& a) {
    hipLaunchKernelGGL(k_trsm_chain16<false>, nb, dim3(256), 0, c->stream, Mb, c->invs, c->invsT, c->y16, c->r16, a);
  };
  chain_launches(c, c->blk_pub, kBlkPub, c->blk_seq, band_w, chain_safe, chain_bw, fwd, bwd);
}

// What the starts of a call on the cached factor share: the state check, the handle's device
inline int call_begin(DirectCore* c) {
  if (!c->factored) {
    c->err = std::string(c->name) + "_solve: no valid factorisation";
    return FPSQ_ERR_STATE;
  }
  hipSetDevice(c->device);
  return FPSQ_OK;
}

// ... and its ends, e0 and e1 being recorded: the synchronisation that makes the outputs complete, the check of the sweeps'
// error word (`expired`: the error text of a wait that ran out), the device time
constexpr const char* kSweepExpired =
    "triangular sweep: a block's solution did not arrive (bounded wait expired); FPSQ_TRSV_CHAIN=0 avoids the path";
inline int call_end(DirectCore* c, const char* expired, double* solve_ms) {
  CHK(c, hipStreamSynchronize(c->stream));
  if (c->chain_err && *c->chain_err) {
    *c->chain_err = 0;
    c->err = expired;
    return FPSQ_ERR_TIMEOUT;
  }
  float ms = 0.f;
  hipEventElapsedTime(&ms, c->e0, c->e1);
  *solve_ms = ms;
  return FPSQ_OK;
}

// Start of a solve_two_* call: argument and state checks, the two right-hand sides staged in in_a / in_b (rhs1: n doubles,
// rhs2: m when `mixed`, else n), e0
inline int solve_begin(DirectCore* c, bool mixed, const double* rhs1, const double* rhs2, const double* p1, const double* q1,
                       const double* p2, const double* q2) {
  if (!c || !rhs1 || !rhs2 || !p1 || !q1 || !p2 || !q2) return FPSQ_ERR_ARG;
  if (int rc = call_begin(c)) return rc;
  CHK(c, hipMemcpyAsync(c->in_a, rhs1, (size_t)c->n * 8, hipMemcpyDefault, c->stream));
  CHK(c, hipMemcpyAsync(c->in_b, rhs2, (size_t)(mixed ? c->m : c->n) * 8, hipMemcpyDefault, c->stream));
  hipEventRecord(c->e0, c->stream);
  return FPSQ_OK;
}

// ... and its end, the results being in flight in o_p1 .. o_q2: e1, the copies to the caller, call_end
inline int solve_end(DirectCore* c, double* p1, double* q1, double* p2, double* q2, double* solve_ms) {
  hipStream_t s = c->stream;
  hipEventRecord(c->e1, s);
  CHK(c, hipMemcpyAsync(p1, c->o_p1, (size_t)c->n * 8, hipMemcpyDefault, s));
  CHK(c, hipMemcpyAsync(p2, c->o_p2, (size_t)c->n * 8, hipMemcpyDefault, s));
  CHK(c, hipMemcpyAsync(q1, c->o_q1, (size_t)c->m * 8, hipMemcpyDefault, s));
  CHK(c, hipMemcpyAsync(q2, c->o_q2, (size_t)c->m * 8, hipMemcpyDefault, s));
  return call_end(c, kSweepExpired, solve_ms);
}

// ---- around the kernels of a device-resident evaluation (fpsq_band_qp_*); nothing here knows how M is stored

inline int set_input_stream(DirectCore* c, int32_t enabled, void* hip_stream) {
  if (!c) return FPSQ_ERR_ARG;
  hipSetDevice(c->device);
  if (enabled && !c->ev_in) CHK(c, hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming));
  c->in_stream_on = enabled != 0;
  c->in_stream = (hipStream_t)hip_stream;
  return FPSQ_OK;
}

// the handle's stream waits (event, no host block) for everything enqueued so far on the registered stream
inline int wait_input(DirectCore* c) {
  if (!c->in_stream_on) return FPSQ_OK;
  CHK(c, hipEventRecord(c->ev_in, c->in_stream));
  CHK(c, hipStreamWaitEvent(c->stream, c->ev_in, 0));
  return FPSQ_OK;
}

// true when p is device memory of the handle's GPU (kernels then use it in place)
inline bool on_device(const DirectCore* c, const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // plain host memory: not an error
    return false;
  }
  return a.type == hipMemoryTypeDevice && a.device == c->device;
}

// An argument of `len` doubles per vector as the kernels see it: the caller's memory when that lives on the handle's GPU
// (stage == null), else a staging buffer that holds one tile of its vectors at a time.  A single vector is one tile of one.
struct StagedArg {
  double* base = nullptr;  // the caller's; null: the argument is absent, and so is its tile
  double* stage = nullptr;
  size_t len = 0;
  double* tile(int v0 = 0) const { return !base ? nullptr : stage ? stage : base + (size_t)v0 * len; }
};

inline StagedArg staged(DirectCore* c, const double* p, double* stage, size_t len) {
  return StagedArg{const_cast<double*>(p), p && !on_device(c, p) ? stage : nullptr, len};
}

// the copy of the caller's vectors v0 .. v0 + kt - 1 into the tile of a staged input / out of the tile of a staged output
inline int stage_in(DirectCore* c, const StagedArg& a, int v0 = 0, int kt = 1) {
  if (a.stage) CHK(c, hipMemcpyAsync(a.stage, a.base + (size_t)v0 * a.len, (size_t)kt * a.len * 8, hipMemcpyDefault, c->stream));
  return FPSQ_OK;
}

inline int stage_back(DirectCore* c, const StagedArg& a, int v0 = 0, int kt = 1) {
  if (a.stage) CHK(c, hipMemcpyAsync(a.base + (size_t)v0 * a.len, a.stage, (size_t)kt * a.len * 8, hipMemcpyDefault, c->stream));
  return FPSQ_OK;
}

// Start of an evaluation on the cached factor: state check, input ordering, e0
inline int eval_begin(DirectCore* c) {
  if (int rc = call_begin(c)) return rc;
  if (int rc = wait_input(c)) return rc;
  hipEventRecord(c->e0, c->stream);
  return FPSQ_OK;
}

// ... and its end: e1, the one device-to-host transfer of the call's `nscal` scalars (c->scal -> c->scal_host), call_end
inline int eval_end(DirectCore* c, int nscal, double* solve_ms, const char* expired = kSweepExpired) {
  hipEventRecord(c->e1, c->stream);
  if (nscal > 0) CHK(c, hipMemcpyAsync(c->scal_host, c->scal, (size_t)nscal * 8, hipMemcpyDeviceToHost, c->stream));
  return call_end(c, expired, solve_ms);
}

// lane_group(nnz, rows) and WITH_LANE_GROUP(lg, ...): fpsq_lanegroup.h (shared with the iterative handle's sparse Hessian)

// ... and with the compile-time constant NAME = the run-time bool `cond`
#define WITH_BOOL(cond, NAME, ...)                   \
  if (cond) { constexpr bool NAME = true; __VA_ARGS__; } \
  else { constexpr bool NAME = false; __VA_ARGS__; }
}  // namespace fpsq_direct
