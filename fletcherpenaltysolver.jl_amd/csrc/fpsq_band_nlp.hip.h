// fpsq_band_nlp.hip.h -- part of the fpsq_band.hip translation unit (included behind the fpsq_band_qp_* group): the
// device-resident model with NONLINEAR equality constraints on the banded handle (C ABI: include/fpsq.h, fpsq_band_nlp_*).
//   f(x) = 1/2 x' diag(q) x + d'x,   c_i(x) = sum_j (A_ij + 1/2 H_ij x_j) x_j - b_i,   H on the pattern of A,
// so J(x)_ij = A_ij + H_ij x_j has the handle's pattern for every x, sum_i y_i Hess c_i = diag(H'y) and
// ghjvprod(x, g, v) = H (g .* v): everything nonlinear is a product with the pattern the handle holds and a second value
// array.  The kernels follow k_bq_* (fpsq_band.hip.h): a lane group per row, grid-stride tiles, sums in a fixed order
// (lanes by xor shuffles, waves and workgroups in index order), no floating-point atomics.
//
// COUPLING TERMS (fpsq_band_nlp_create_coupled) add sum_{t in i} w_t x_jt x_kt to c_i, jt != kt both columns of row i of A, so
// J(x)_ij = A_ij + H_ij x_j + sum w_t x_partner keeps the handle's pattern, sum_i y_i Hess c_i = diag(H'y) + Wo(y) with Wo(y)
// sparse symmetric on a pattern S fixed at create, and ghjvprod gains w_t (g_j v_k + g_k v_j).  The index lists come from
// fpsq_coupled.h.  The model's `lin` view carries S and -Wo(ys) as the R of a sparse objective Hessian, so hprod Val(2) is
// bq_launches' sparse form with Q = diag(qe) - Wo(ys), unchanged.  It is ONE model: the kernels that walk a row of A or of A'
// take the terms as the compile-time flag CP (one row walk, `if constexpr` where an expression differs), the kernels on the
// lists and on S (k_bcn_*) have no separable counterpart, and the drivers branch only where a launch differs.
// fpsq_band_nlp_create_coupled_arrow puts the terms on handles with border rows and long columns: border rows and the entries of
// long columns are ordinary stored entries to every kernel on the stored CSR and on the lists; the virtual transposed entries
// of a long column meet no term; and the row of S a long column owns (up to m entries) is listed apart from the CSR the
// lane-group kernels walk and summed by one workgroup (k_bq_long_rows, fpsq_band.hip.h "LONG ROWS").
#pragma once
#include <limits>

#include "fpsq_coupled.h"

namespace fpsq {

// the partner lists of the entries of one CSR (fpsq_coupled.h): entry k meets x[col[u]] with weight w[u], u in
// [ptr[k], ptr[k + 1]).  What only the CP forms of the row kernels read; all null on a model without terms.
struct bn_partners {
  const int32_t *ptr, *col;
  const double* w;
};

// vals[k] = a[k] + h[k] x[colind[k]] over the stored CSR: J(x) where k_band_form_t and the A products read it
__global__ __launch_bounds__(256) void k_bn_vals(const double* __restrict__ a, const double* __restrict__ h,
                                                 const int32_t* __restrict__ colind, const double* __restrict__ x,
                                                 double* __restrict__ vals, int64_t nnz) {
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < nnz; k += (int64_t)gridDim.x * 256)
    vals[k] = a[k] + h[k] * x[colind[k]];
}

// The same in the transposed CSR, a lane group per row j (a column of J): t_vals[k] = ta[k] + th[k] x[j]; x_j is read once
// per row, nothing is gathered
template <int LG>
__global__ __launch_bounds__(256) void k_bn_tvals(const int32_t* __restrict__ t_rowptr, const double* __restrict__ ta,
                                                  const double* __restrict__ th, const double* __restrict__ x,
                                                  double* __restrict__ t_vals, int n) {
  constexpr int RPB = 256 / LG;
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  const int ntiles = (n + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int j = tile * RPB + g;
    if (j >= n) continue;
    const double xv = x[j];
    const int e = t_rowptr[j + 1];
    for (int k = t_rowptr[j] + l; k < e; k += LG) t_vals[k] = ta[k] + th[k] * xv;
  }
}

// ---- FUNCTION TERMS (fpsq_band_nlp_create_fn): c_i(x) = sum_j (A_ij x_j + H_ij phi_kij(x_j)) - b_i with phi from the table
// FPSQ_FN_* (include/fpsq.h), one code byte per entry.  J(x)_ij = A_ij + H_ij phi'(x_j) keeps the pattern and the curvature
// coefficient becomes an array every objgrad rewrites, G(x)_ij = H_ij phi''(x_j): the kernels that read h / th next to J
// (k_bn_epilogue, k_bn_epilogue_h1, k_bn_hgv, the long-column sums) are handed g / tg and stay as they are.  New are the two
// value kernels below and the forms of the prologue (FN) and of k_bn_cons that no longer know c from J by the quadratic identity.

// phi, phi', phi'' of function `code` at x.  ONE device function and one expression for every kernel that needs a value, with
// contraction off, so that the stored and the transposed value arrays get the same bits whatever surrounds the call
__device__ __forceinline__ void bn_fn_eval(int code, double x, double& p0, double& p1, double& p2) {
#pragma clang fp contract(off)
  switch (code) {
    case FPSQ_FN_HALFSQ:
      p1 = x;
      p2 = 1.0;
      p0 = 0.5 * x * x;
      break;
    case FPSQ_FN_CUBE6:
      p2 = x;
      p1 = 0.5 * x * x;
      p0 = p1 * x * (1.0 / 3.0);
      break;
    case FPSQ_FN_SIN: {
      const double sv = sin(x);
      p0 = sv;
      p1 = cos(x);
      p2 = -sv;
    } break;
    case FPSQ_FN_COS: {
      const double cv = cos(x);
      p0 = cv;
      p1 = -sin(x);
      p2 = -cv;
    } break;
    case FPSQ_FN_EXP:
      p0 = p1 = p2 = exp(x);
      break;
    default: {  // FPSQ_FN_TANH (the create entry refuses every other code)
      const double tv = tanh(x), uv = 1.0 - tv * tv;
      p0 = tv;
      p1 = uv;
      p2 = -2.0 * tv * uv;
    } break;
  }
}

// the J value and the curvature coefficient of one entry from its function's derivatives (both value kernels)
__device__ __forceinline__ void bn_fn_jg(double a, double h, double p1, double p2, double& jv, double& gv) {
#pragma clang fp contract(off)
  jv = a + h * p1;
  gv = h * p2;
}

// The function form of k_bn_vals: vals[k] = a[k] + h[k] phi'(x_c) (J(x)), g[k] = h[k] phi''(x_c) (G(x)) and the remainder
// rem[k] = h[k] (phi'(x_c) x_c - phi(x_c)), with which the prologue has c_p = sum_k (J_k x_c - rem_k) - b_p.  A non-finite J value
// (exp overflows above 709) raises *flag: every thread that sees one stores the same 1, the driver reads the word before it
// factorises and clears it after it has fired
__global__ __launch_bounds__(256) void k_bn_vals_fn(const double* __restrict__ a, const double* __restrict__ h,
                                                    const uint8_t* __restrict__ code, const int32_t* __restrict__ colind,
                                                    const double* __restrict__ x, double* __restrict__ vals,
                                                    double* __restrict__ g, double* __restrict__ rem, int32_t* __restrict__ flag,
                                                    int64_t nnz) {
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < nnz; k += (int64_t)gridDim.x * 256) {
    const double xv = x[colind[k]], hv = h[k];
    double p0, p1, p2, jv, gv;
    bn_fn_eval(code[k], xv, p0, p1, p2);
    bn_fn_jg(a[k], hv, p1, p2, jv, gv);
    vals[k] = jv;
    g[k] = gv;
    rem[k] = hv * (p1 * xv - p0);
    if (!isfinite(jv)) *flag = 1;
  }
}

// The function form of k_bn_tvals, a lane group per row j: t_vals[k] = ta[k] + th[k] phi'(x_j), tg[k] = th[k] phi''(x_j).  x_j is
// read once per row and phi', phi'' are evaluated once per function code PRESENT in the row (the lanes' code bits joined by xor
// shuffles), not per entry; an entry picks its pair by its code.  The virtual entries of a long column have code 0, ta = 1,
// th = 0: J' gathers 1 and G' is 0 there
template <int LG>
__global__ __launch_bounds__(256) void k_bn_tvals_fn(const int32_t* __restrict__ t_rowptr, const double* __restrict__ ta,
                                                     const double* __restrict__ th, const uint8_t* __restrict__ tcode,
                                                     const double* __restrict__ x, double* __restrict__ t_vals,
                                                     double* __restrict__ tg, int n) {
  constexpr int RPB = 256 / LG;
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  const int ntiles = (n + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int j = tile * RPB + g;
    int lo = 0, e = 0;
    double xv = 0.0;
    if (j < n) {
      xv = x[j];
      lo = t_rowptr[j];
      e = t_rowptr[j + 1];
    }
    int present = 0;
    for (int k = lo + l; k < e; k += LG) present |= 1 << tcode[k];
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) present |= __shfl_xor(present, o);
    double d1[FPSQ_FN_COUNT], d2[FPSQ_FN_COUNT];
#pragma unroll
    for (int c = 0; c < FPSQ_FN_COUNT; ++c) {
      d1[c] = d2[c] = 0.0;
      if ((present >> c) & 1) {
        double p0;
        bn_fn_eval(c, xv, p0, d1[c], d2[c]);
      }
    }
    for (int k = lo + l; k < e; k += LG) {
      const int code = tcode[k];
      double p1 = d1[0], p2 = d2[0];
#pragma unroll
      for (int c = 1; c < FPSQ_FN_COUNT; ++c) {
        p1 = code == c ? d1[c] : p1;
        p2 = code == c ? d2[c] : p2;
      }
      double jv, gv;
      bn_fn_jg(ta[k], th[k], p1, p2, jv, gv);
      t_vals[k] = jv;
      tg[k] = gv;
    }
  }
}

// ---- FUNCTION TERMS IN THE OBJECTIVE (fpsq_band_nlp_set_objective_terms): f(x) = 1/2 x' diag(q) x + d'x + sum_j w_j psi_kj(x_j),
// psi from the same table by one code byte per VARIABLE.  grad f = q x + d + w psi'(x) and Hess f = diag(q + w psi''(x)), and
// q and d enter an objgrad only through k_bq_pack<false>, k_bn_epilogue and k_bn_lc_epilogue (the Hessian products read qe, hc
// and gs): this kernel rewrites two EFFECTIVE vectors per objgrad,
//   qx_j = q_j + w_j psi''(x_j),   de_j = d_j + w_j (psi'(x_j) - psi''(x_j) x_j),   so that qx_j x_j + de_j = grad f(x)_j,
// and those kernels take (qx, de) where they take (q, d), unchanged.  part[blk] = this workgroup's slice of f, over the chunk
// of the prologue's objective slice (contiguous, ceil(n / grid) entries), summed in a fixed order; k_bq_phi_sq finishes fx from
// it.  An entry with w_j = 0 is not evaluated (qx_j = q_j, de_j = d_j: exp at 800 under w_j = 0 is harmless).  A non-finite
// w psi, w psi' or w psi'' raises bit 1 of *flag (k_bn_vals_fn stores 1 there, and has run before this launch); the driver
// reads the word before it factorises
__global__ __launch_bounds__(256) void k_bn_objfn(const double* __restrict__ x, const double* __restrict__ q,
                                                  const double* __restrict__ d, const double* __restrict__ w,
                                                  const uint8_t* __restrict__ code, double* __restrict__ qx,
                                                  double* __restrict__ de, double* __restrict__ part, int32_t* __restrict__ flag,
                                                  int n) {
  __shared__ double sh[4];
  double red[1] = {0.0};
  const int64_t chunk = ((int64_t)n + gridDim.x - 1) / gridDim.x;
  const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
  for (int64_t j = lo + threadIdx.x; j < hi; j += 256) {
    const double xv = x[j], qv = q[j], dv = d[j], wv = w[j];
    double f = xv * (0.5 * qv * xv + dv), qo = qv, eo = dv;
    if (wv != 0.0) {
      double p0, p1, p2;
      bn_fn_eval(code[j], xv, p0, p1, p2);
      const double t0 = wv * p0, t1 = wv * p1, t2 = wv * p2;
      if (!(isfinite(t0) && isfinite(t1) && isfinite(t2))) atomicOr(flag, 2);
      f += t0;
      qo = qv + t2;
      eo = dv + wv * (p1 - p2 * xv);
    }
    qx[j] = qo;
    de[j] = eo;
    red[0] += f;
  }
  bq_block_sum(red, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// With coupling terms: vals[k] = a[k] + h[k] x[col[k]] + sum_u pw[u] x[pcol[u]] over the entries of ONE CSR and their partner
// lists: launched on the stored structure (col = colind) and on the transposed one (col = the entry's own column, its lists in
// the same order), so both value arrays get the same bits
__global__ __launch_bounds__(256) void k_bcn_vals(const double* __restrict__ a, const double* __restrict__ h,
                                                  const int32_t* __restrict__ col, const int32_t* __restrict__ pptr,
                                                  const int32_t* __restrict__ pcol, const double* __restrict__ pw,
                                                  const double* __restrict__ x, double* __restrict__ vals, int64_t nnz) {
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < nnz; k += (int64_t)gridDim.x * 256) {
    double s = a[k] + h[k] * x[col[k]];
    const int e = pptr[k + 1];
    for (int u = pptr[k]; u < e; ++u) s += pw[u] * x[pcol[u]];
    vals[k] = s;
  }
}

// The prologue of an objgrad: one pass over the stored CSR reading J (vals), a second value array and the packed pair
// xg[c] = {g_c, x_c} (k_bq_pack<false>): r[p] = {(J g)_p, -c_p} where the sweeps read it (zero on the padding), keep[p] = c_p;
// part[2 blk] = this workgroup's slice of f = x.(1/2 q x + d), part[2 blk + 1] = of c.c.  Separable: ha = h and
// c_p = sum (J - 1/2 h x_c) x_c - b_p.  CP: ha = a and c_p = sum 1/2 (J + a) x_c - b_p, which holds for a symmetric curvature of
// any kind and needs no walk of the term lists (J = vals already holds them).  FN (function terms): ha = rem and
// c_p = sum (J x_c - rem) - b_p, the remainder k_bn_vals_fn left next to J.
template <int LG, bool CP, bool FN = false>
__global__ __launch_bounds__(256) void k_bn_prologue(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                     const double* __restrict__ vals, const double* __restrict__ ha,
                                                     const double* __restrict__ xg, const double* __restrict__ x,
                                                     const double* __restrict__ q, const double* __restrict__ d,
                                                     const double* __restrict__ bp, double* __restrict__ r,
                                                     double* __restrict__ keep, double* __restrict__ part, int m, int mpad,
                                                     int n) {
  constexpr int RPB = 256 / LG;
  __shared__ double sh[8];
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  double red[2] = {0.0, 0.0};
  const int ntiles = (mpad + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int p = tile * RPB + g;
    double a0 = 0.0, a1 = 0.0;
    if (p < m) {
      const int e = rowptr[p + 1];
      for (int k = rowptr[p] + l; k < e; k += LG) {
        const double jv = vals[k], hv = ha[k], av = hv;  // (the one array under the name each form knows it by)
        const f64x2 t = *reinterpret_cast<const f64x2*>(xg + (size_t)colind[k] * 2);
        a0 += jv * t.x;
        if constexpr (FN)
          a1 += jv * t.y - hv;
        else if constexpr (CP)
          a1 += (0.5 * (jv + av)) * t.y;
        else
          a1 += (jv - 0.5 * hv * t.y) * t.y;
      }
    }
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) {
      a0 += __shfl_xor(a0, o);
      a1 += __shfl_xor(a1, o);
    }
    if (l == 0 && p < mpad) {  // (a0 = a1 = 0 on the padding rows)
      double cv = 0.0, r1 = 0.0;
      if (p < m) {
        cv = a1 - bp[p];
        r1 = -cv;
        red[1] += cv * cv;
      }
      *reinterpret_cast<f64x2*>(r + (size_t)p * 2) = f64x2{a0, r1};
      keep[p] = cv;
    }
  }
  const int64_t chunk = ((int64_t)n + gridDim.x - 1) / gridDim.x;
  const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
  for (int64_t j = lo + threadIdx.x; j < hi; j += 256) {
    const double xv = x[j];
    red[0] += xv * (0.5 * q[j] * xv + d[j]);
  }
  bq_block_sum(red, sh);
  if (threadIdx.x == 0) {
    part[(size_t)blockIdx.x * 2] = red[0];
    part[(size_t)blockIdx.x * 2 + 1] = red[1];
  }
}

// c(x) alone, from the model's own arrays (no factorisation has to have put J into the handle), in the caller's row order
// (rperm: stored row -> the caller's, null = identity): c_p = sum (a + 1/2 h x_c) x_c - b_p; CP:
// c_p = sum (a + 1/2 h x_c + 1/2 sum_u w x_partner) x_c - b_p (every term is met at both of its entries, half each)
template <int LG, bool CP>
__global__ __launch_bounds__(256) void k_bn_cons(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                 const double* __restrict__ a, const double* __restrict__ h,
                                                 const double* __restrict__ x, const double* __restrict__ bp,
                                                 const int32_t* __restrict__ rperm, double* __restrict__ c, int m,
                                                 bn_partners pt) {
  [[maybe_unused]] const int32_t *__restrict__ pptr = pt.ptr, *__restrict__ pcol = pt.col;
  [[maybe_unused]] const double* __restrict__ pw = pt.w;
  constexpr int RPB = 256 / LG;
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  const int ntiles = (m + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int p = tile * RPB + g;
    double s = 0.0;
    if (p < m) {
      const int e = rowptr[p + 1];
      for (int k = rowptr[p] + l; k < e; k += LG) {
        const double xv = x[colind[k]];
        if constexpr (CP) {
          double ps = 0.0;
          const int ue = pptr[k + 1];
          for (int u = pptr[k]; u < ue; ++u) ps += pw[u] * x[pcol[u]];
          s += (a[k] + 0.5 * h[k] * xv + 0.5 * ps) * xv;
        } else {
          s += (a[k] + 0.5 * h[k] * xv) * xv;
        }
      }
    }
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (l == 0 && p < m) c[rperm ? rperm[p] : p] = s - bp[p];
  }
}

// The function form of k_bn_cons: c_p = sum (a x_c + h phi(x_c)) - b_p from the model's own arrays and code bytes
template <int LG>
__global__ __launch_bounds__(256) void k_bn_cons_fn(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                    const double* __restrict__ a, const double* __restrict__ h,
                                                    const uint8_t* __restrict__ code, const double* __restrict__ x,
                                                    const double* __restrict__ bp, const int32_t* __restrict__ rperm,
                                                    double* __restrict__ c, int m) {
  constexpr int RPB = 256 / LG;
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  const int ntiles = (m + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int p = tile * RPB + g;
    double s = 0.0;
    if (p < m) {
      const int e = rowptr[p + 1];
      for (int k = rowptr[p] + l; k < e; k += LG) {
        const double xv = x[colind[k]];
        double p0, p1, p2;
        bn_fn_eval(code[k], xv, p0, p1, p2);
        s += a[k] * xv + h[k] * p0;
      }
    }
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (l == 0 && p < m) c[rperm ? rperm[p] : p] = s - bp[p];
  }
}

// The epilogue of an objgrad: one pass over the transposed CSR reading TWO value arrays (J' = t_vals, H' = th) against three
// m-vectors (y[p] = {q1, q2}, keep = c), six sums per row j: s1 = (J'q1)_j, s2 = (J'q2)_j, s3 = (J'c)_j, h1 = (H'q1)_j,
// h2 = (H'q2)_j, h3 = (H'c)_j.  With g_j = q_j x_j + d_j:
//   gs_j = g_j - s1 - sigma s2,  p2_j = -s2,  qe_j = q_j - (h1 + sigma h2) = (q - H'ys)_j,  hc_j = h3,
//   gx_j = gs_j - qe_j p2_j + sigma p2_j + h2 gs_j + rho s3 + eta (x_j - xk_j)       (the gradient in the -ys form)
// qe, hc, gsm (the model's own copies, what fpsq_band_nlp_hprod runs on) are always written; out, gs, ys, xk may be null.
// ys and the partials part[2 blk] = slice of c.ys, part[2 blk + 1] = of |x - xk|^2 as in k_bq_epilogue.
// CP also leaves p2_j in tv: its gx_j lacks Wo(ys) p2 + Wo(q2) gs, whose rows need every p2 and gs (k_bcn_finish adds them).
template <int LG, bool CP>
__global__ __launch_bounds__(256) void k_bn_epilogue(const int32_t* __restrict__ t_rowptr, const int32_t* __restrict__ t_colind,
                                                     const double* __restrict__ t_vals, const double* __restrict__ th,
                                                     const double* __restrict__ y, const double* __restrict__ keep,
                                                     const int32_t* __restrict__ rperm, const double* __restrict__ x,
                                                     const double* __restrict__ xk, const double* __restrict__ q,
                                                     const double* __restrict__ d, double sigma, double rho, double eta,
                                                     double* __restrict__ out, double* __restrict__ gs, double* __restrict__ ys,
                                                     double* __restrict__ qe, double* __restrict__ hc, double* __restrict__ gsm,
                                                     double* __restrict__ tv, double* __restrict__ part, int n, int m) {
  constexpr int RPB = 256 / LG;
  __shared__ double sh[8];
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  double red[2] = {0.0, 0.0};
  const int ntiles = (n + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int j = tile * RPB + g;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0, h1 = 0.0, h2 = 0.0, h3 = 0.0;
    if (j < n) {
      const int e = t_rowptr[j + 1];
      for (int k = t_rowptr[j] + l; k < e; k += LG) {
        const double jv = t_vals[k], hv = th[k];
        const int p = t_colind[k];
        const f64x2 t = *reinterpret_cast<const f64x2*>(y + (size_t)p * 2);
        const double cv = keep[p];
        s1 += jv * t.x;
        s2 += jv * t.y;
        s3 += jv * cv;
        h1 += hv * t.x;
        h2 += hv * t.y;
        h3 += hv * cv;
      }
    }
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) {
      s1 += __shfl_xor(s1, o);
      s2 += __shfl_xor(s2, o);
      s3 += __shfl_xor(s3, o);
      h1 += __shfl_xor(h1, o);
      h2 += __shfl_xor(h2, o);
      h3 += __shfl_xor(h3, o);
    }
    if (l == 0 && j < n) {
      const double xv = x[j], qv = q[j];
      const double gsv = (qv * xv + d[j]) - s1 - sigma * s2, p2 = -s2;
      const double qev = qv - (h1 + sigma * h2);
      const double dx = eta > 0.0 ? xv - (xk ? xk[j] : 0.0) : 0.0;
      qe[j] = qev;
      hc[j] = h3;
      gsm[j] = gsv;
      if constexpr (CP) tv[j] = p2;
      if (gs) gs[j] = gsv;
      if (out) out[j] = gsv + (sigma - qev) * p2 + h2 * gsv + rho * s3 + eta * dx;
      red[1] += dx * dx;
    }
  }
  const int64_t chunk = ((int64_t)m + gridDim.x - 1) / gridDim.x;
  const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < m ? lo + chunk : m;
  for (int64_t p = lo + threadIdx.x; p < hi; p += 256) {
    const f64x2 t = *reinterpret_cast<const f64x2*>(y + (size_t)p * 2);
    const double yv = t.x + sigma * t.y;
    if (ys) ys[rperm ? rperm[p] : p] = yv;
    red[0] += keep[p] * yv;
  }
  bq_block_sum(red, sh);
  if (threadIdx.x == 0) {
    part[(size_t)blockIdx.x * 2] = red[0];
    part[(size_t)blockIdx.x * 2 + 1] = red[1];
  }
}

// With coupling terms, behind the epilogue: the values of -Wo(ys), Wo(q2), Wo(c) on S in one pass over the contributor lists
// (increasing stored row): y[p] = {q1, q2} the sweeps' solution, keep = c, ys_p = q1 + sigma q2 as the epilogue forms it.
// rv = -Wo(ys) is the R of the model's `lin` view.
__global__ __launch_bounds__(256) void k_bcn_assemble(const int32_t* __restrict__ cptr, const int32_t* __restrict__ crow,
                                                      const double* __restrict__ cw, const double* __restrict__ y,
                                                      const double* __restrict__ keep, double sigma, double* __restrict__ rv,
                                                      double* __restrict__ wq2, double* __restrict__ wc, int64_t snz) {
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < snz; k += (int64_t)gridDim.x * 256) {
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    const int e = cptr[k + 1];
    for (int u = cptr[k]; u < e; ++u) {
      const int p = crow[u];
      const double w = cw[u];
      const f64x2 t = *reinterpret_cast<const f64x2*>(y + (size_t)p * 2);
      s1 += w * (t.x + sigma * t.y);
      s2 += w * t.y;
      s3 += w * keep[p];
    }
    rv[k] = -s1;
    wq2[k] = s2;
    wc[k] = s3;
  }
}

// gx_j += sum_k (Wo(q2)_jk gs_k + Wo(ys)_jk p2_k) over row j of S, a lane group per row
template <int LG>
__global__ __launch_bounds__(256) void k_bcn_finish(const int32_t* __restrict__ srp, const int32_t* __restrict__ sci,
                                                    const double* __restrict__ rv, const double* __restrict__ wq2,
                                                    const double* __restrict__ p2, const double* __restrict__ gsm,
                                                    double* __restrict__ out, int n) {
  constexpr int RPB = 256 / LG;
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  const int ntiles = (n + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int j = tile * RPB + g;
    double s = 0.0;
    if (j < n) {
      const int e = srp[j + 1];
      for (int k = srp[j] + l; k < e; k += LG) {
        const int c = sci[k];
        s += wq2[k] * gsm[c] - rv[k] * p2[c];
      }
    }
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (l == 0 && j < n) out[j] += s;
  }
}

// hprod Val(2), behind the unchanged k_bq_epilogue<LG, true> (q = qe): Hv += hc .* v   (:560-562: Hcv is not scaled by rho)
__global__ __launch_bounds__(256) void k_bn_hcv(const double* __restrict__ hc, const double* __restrict__ v,
                                                double* __restrict__ Hv, int n) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < n) Hv[j] += hc[j] * v[j];
}

// The same with coupling terms, behind bq_launches' sparse form (Q = diag(qe) - Wo(ys)): Hv_j += hc_j v_j + (Wo(c) v)_j
template <int LG>
__global__ __launch_bounds__(256) void k_bcn_hcv(const int32_t* __restrict__ srp, const int32_t* __restrict__ sci,
                                                 const double* __restrict__ wc, const double* __restrict__ hc,
                                                 const double* __restrict__ v, double* __restrict__ Hv, int n) {
  constexpr int RPB = 256 / LG;
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  const int ntiles = (n + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int j = tile * RPB + g;
    double s = 0.0;
    if (j < n) {
      const int e = srp[j + 1];
      for (int k = srp[j] + l; k < e; k += LG) s += wc[k] * v[sci[k]];
    }
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (l == 0 && j < n) Hv[j] += hc[j] * v[j] + s;
  }
}

// The epilogue of an hprod Val(1) (:572-634): the hprod rows of k_bq_epilogue with q = qe -- y[p] = {q1, q2} the solutions
// for {J v, J (qe v)}, keep = J v; s1 = (J'q1)_j = Ptv_j, s2 = (J'q2)_j, s3 = (J'J v)_j -- and a fourth sum h1 = (H'q1)_j:
//   Hv_j = (qe_j v_j - s2) - qe_j s1 + 2 sigma s1 + rho (s3 + hc_j v_j) + eta v_j - h1 gs_j        (:612-614, :626)
// CP has E = diag(qe) - Wo(ys) in the place of qe: vx is not v but the packed pair xg[j] = {v_j, (E v)_j} of k_bq_pack_sq<HP>
// (the second solve's right-hand side was J (E v)), (E v)_j stands where qe_j v_j does, and Ptv_j = s1 is left in tv for
// k_bcn_finish_h1.
template <int LG, bool CP>
__global__ __launch_bounds__(256) void k_bn_epilogue_h1(const int32_t* __restrict__ t_rowptr, const int32_t* __restrict__ t_colind,
                                                        const double* __restrict__ t_vals, const double* __restrict__ th,
                                                        const double* __restrict__ y, const double* __restrict__ keep,
                                                        const double* __restrict__ vx, const double* __restrict__ qe,
                                                        const double* __restrict__ hc, const double* __restrict__ gsm,
                                                        double sigma, double rho, double eta, double* __restrict__ out,
                                                        double* __restrict__ tv, int n) {
  constexpr int RPB = 256 / LG;
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  const int ntiles = (n + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int j = tile * RPB + g;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0, h1 = 0.0;
    if (j < n) {
      const int e = t_rowptr[j + 1];
      for (int k = t_rowptr[j] + l; k < e; k += LG) {
        const double jv = t_vals[k];
        const int p = t_colind[k];
        const f64x2 t = *reinterpret_cast<const f64x2*>(y + (size_t)p * 2);
        s1 += jv * t.x;
        s2 += jv * t.y;
        s3 += jv * keep[p];
        h1 += th[k] * t.x;
      }
    }
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) {
      s1 += __shfl_xor(s1, o);
      s2 += __shfl_xor(s2, o);
      s3 += __shfl_xor(s3, o);
      h1 += __shfl_xor(h1, o);
    }
    if (l == 0 && j < n) {
      if constexpr (CP) {
        const f64x2 t = *reinterpret_cast<const f64x2*>(vx + (size_t)j * 2);
        const double vv = t.x, qv = qe[j];
        out[j] = (t.y - s2) - qv * s1 + 2.0 * sigma * s1 + rho * (s3 + hc[j] * vv) + eta * vv - h1 * gsm[j];
        tv[j] = s1;
      } else {
        const double vv = vx[j], qv = qe[j];
        out[j] = (qv * vv - s2) - qv * s1 + 2.0 * sigma * s1 + rho * (s3 + hc[j] * vv) + eta * vv - h1 * gsm[j];
      }
    }
  }
}

// hprod Val(1) with coupling terms, the rows of S: Hv_j += sum_k (Wo(ys)_jk Ptv_k + rho Wo(c)_jk v_k - Wo(q1)_jk gs_k).  Wo(q1)
// is used once, so its entries are summed here from the contributor lists and the first solve's y[p] = {q1, .} (before the
// second solve takes y)
template <int LG>
__global__ __launch_bounds__(256) void k_bcn_finish_h1(const int32_t* __restrict__ srp, const int32_t* __restrict__ sci,
                                                       const int32_t* __restrict__ cptr, const int32_t* __restrict__ crow,
                                                       const double* __restrict__ cw, const double* __restrict__ rv,
                                                       const double* __restrict__ wc, const double* __restrict__ y,
                                                       const double* __restrict__ tv, const double* __restrict__ v,
                                                       const double* __restrict__ gsm, double rho, double* __restrict__ out,
                                                       int n) {
  constexpr int RPB = 256 / LG;
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  const int ntiles = (n + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int j = tile * RPB + g;
    double s = 0.0;
    if (j < n) {
      const int e = srp[j + 1];
      for (int k = srp[j] + l; k < e; k += LG) {
        const int c = sci[k];
        double wq1 = 0.0;
        const int ue = cptr[k + 1];
        for (int u = cptr[k]; u < ue; ++u) wq1 += cw[u] * y[(size_t)crow[u] * 2];
        s += (rho * wc[k]) * v[c] - rv[k] * tv[c] - wq1 * gsm[c];
      }
    }
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (l == 0 && j < n) out[j] += s;
  }
}

// Ssv = ghjvprod(x, gs, v) = H (gs .* v) (:600) over the stored CSR, straight into the sweeps' right-hand-side layout:
// r[p] = {Ssv_p, 0}, zero on the padding.  CP: with the terms, Ssv_p = sum_k gs_c (h_k v_c + sum_u w v_partner)
template <int LG, bool CP>
__global__ __launch_bounds__(256) void k_bn_hgv(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                const double* __restrict__ h, const double* __restrict__ gsm,
                                                const double* __restrict__ v, double* __restrict__ r, int m, int mpad,
                                                bn_partners pt) {
  [[maybe_unused]] const int32_t *__restrict__ pptr = pt.ptr, *__restrict__ pcol = pt.col;
  [[maybe_unused]] const double* __restrict__ pw = pt.w;
  constexpr int RPB = 256 / LG;
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  const int ntiles = (mpad + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int p = tile * RPB + g;
    double s = 0.0;
    if (p < m) {
      const int e = rowptr[p + 1];
      for (int k = rowptr[p] + l; k < e; k += LG) {
        const int c = colind[k];
        if constexpr (CP) {
          double t = h[k] * v[c];
          const int ue = pptr[k + 1];
          for (int u = pptr[k]; u < ue; ++u) t += pw[u] * v[pcol[u]];
          s += gsm[c] * t;
        } else {
          s += h[k] * (gsm[c] * v[c]);
        }
      }
    }
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (l == 0 && p < mpad) *reinterpret_cast<f64x2*>(r + (size_t)p * 2) = f64x2{s, 0.0};
  }
}

// out_j -= (J'z)_j with z = column 0 of the sweeps' solution y[p] = {z_p, .}   (:606, :612)
template <int LG>
__global__ __launch_bounds__(256) void k_bn_jtz(const int32_t* __restrict__ t_rowptr, const int32_t* __restrict__ t_colind,
                                                const double* __restrict__ t_vals, const double* __restrict__ y,
                                                double* __restrict__ out, int n) {
  constexpr int RPB = 256 / LG;
  const int g = threadIdx.x / LG, l = threadIdx.x % LG;
  const int ntiles = (n + RPB - 1) / RPB;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int j = tile * RPB + g;
    double s = 0.0;
    if (j < n) {
      const int e = t_rowptr[j + 1];
      for (int k = t_rowptr[j] + l; k < e; k += LG) s += t_vals[k] * y[(size_t)t_colind[k] * 2];
    }
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (l == 0 && j < n) out[j] -= s;
  }
}

// ---- long columns (fpsq_band_nlp_create_arrow).  In the transposed structure long column i (column j = lcols[i]) has no real
// entries: its vgrid virtual entries gather the value 1 (ta = 1, th = 0) and point at the virtual rows mpad + 16 g + i, where
// the solutions hold w (g = 0, zero elsewhere) and `keep` the chunk sums of U'keep.  The J' sums of the kernels above are
// therefore complete at j; the H' sums come out 0.  These two kernels form them from h over the column's own entries, ONE
// WORKGROUP PER LONG COLUMN behind the epilogue, and write that row's outputs again.  Sums in a fixed order (a thread's entries
// in index order, lanes by xor shuffles, waves in index order), no atomics.

// six sums of long column i over the workgroup, in thread 0: v[0 .. 2] = (J'q1)_j, (J'q2)_j, (J'keep)_j from the virtual rows,
// v[3 .. 5] = (H'q1)_j, (H'q2)_j, (H'keep)_j from h
__device__ __forceinline__ void bn_lc_sums(const int32_t* __restrict__ lc_ptr, const int32_t* __restrict__ lc_row,
                                           const int32_t* __restrict__ lc_ent, const double* __restrict__ h,
                                           const double* __restrict__ y, const double* __restrict__ keep, int mpad, int vgrid,
                                           double (&v)[6], double* sh) {
  const int i = blockIdx.x;
#pragma unroll
  for (int k = 0; k < 6; ++k) v[k] = 0.0;
  for (int g = threadIdx.x; g < vgrid; g += 256) {
    const size_t row = (size_t)mpad + (size_t)kBorderMax * g + i;
    const f64x2 t = *reinterpret_cast<const f64x2*>(y + row * 2);
    v[0] += t.x;
    v[1] += t.y;
    v[2] += keep[row];
  }
  const int e = lc_ptr[i + 1];
  int k = lc_ptr[i] + threadIdx.x;
  // four entries of a thread per trip: their (dependent, gathered) loads are in flight together; the terms enter the sums in
  // the order of the one-entry loop behind it
  for (; k + 3 * 256 < e; k += 4 * 256) {
    double hv[4], kv[4];
    f64x2 t[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int p = lc_row[k + u * 256];
      hv[u] = h[lc_ent[k + u * 256]];
      t[u] = *reinterpret_cast<const f64x2*>(y + (size_t)p * 2);
      kv[u] = keep[p];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      v[3] += hv[u] * t[u].x;
      v[4] += hv[u] * t[u].y;
      v[5] += hv[u] * kv[u];
    }
  }
  for (; k < e; k += 256) {
    const double hv = h[lc_ent[k]];
    const int p = lc_row[k];
    const f64x2 t = *reinterpret_cast<const f64x2*>(y + (size_t)p * 2);
    v[3] += hv * t.x;
    v[4] += hv * t.y;
    v[5] += hv * keep[p];
  }
  bq_block_sum(v, sh);
}

// objgrad, behind k_bn_epilogue (which left qe_j = q_j, hc_j = 0 and gx_j without the curvature terms at a long column; gs_j
// and gsm_j hold no H' sum and stay): qe_j, hc_j and gx_j by k_bn_epilogue's formulas with the sums above
__global__ __launch_bounds__(256) void k_bn_lc_epilogue(const int32_t* __restrict__ lc_ptr, const int32_t* __restrict__ lc_row,
                                                        const int32_t* __restrict__ lc_ent, const int32_t* __restrict__ lcols,
                                                        const double* __restrict__ h, const double* __restrict__ y,
                                                        const double* __restrict__ keep, const double* __restrict__ x,
                                                        const double* __restrict__ xk, const double* __restrict__ q,
                                                        const double* __restrict__ gsm, double sigma, double rho, double eta,
                                                        double* __restrict__ out, double* __restrict__ qe,
                                                        double* __restrict__ hc, int mpad, int vgrid) {
  __shared__ double sh[24];
  double v[6];
  bn_lc_sums(lc_ptr, lc_row, lc_ent, h, y, keep, mpad, vgrid, v, sh);
  if (threadIdx.x == 0) {
    const int j = lcols[blockIdx.x];
    const double gsv = gsm[j], p2 = -v[1];
    const double qev = q[j] - (v[3] + sigma * v[4]);
    const double dx = eta > 0.0 ? x[j] - (xk ? xk[j] : 0.0) : 0.0;
    qe[j] = qev;
    hc[j] = v[5];
    if (out) out[j] = gsv + (sigma - qev) * p2 + v[4] * gsv + rho * v[2] + eta * dx;
  }
}

// hprod Val(1), behind k_bn_epilogue_h1 (whose h1 is 0 at a long column): Hv_j by its formula with the sums above.  CP: as
// k_bn_epilogue_h1<LG, true>, vec is the packed pair xg[j] = {v_j, (E v)_j} and (E v)_j stands where qe_j v_j does
template <bool CP>
__global__ __launch_bounds__(256) void k_bn_lc_epilogue_h1(const int32_t* __restrict__ lc_ptr, const int32_t* __restrict__ lc_row,
                                                           const int32_t* __restrict__ lc_ent, const int32_t* __restrict__ lcols,
                                                           const double* __restrict__ h, const double* __restrict__ y,
                                                           const double* __restrict__ keep, const double* __restrict__ vec,
                                                           const double* __restrict__ qe, const double* __restrict__ hc,
                                                           const double* __restrict__ gsm, double sigma, double rho, double eta,
                                                           double* __restrict__ out, int mpad, int vgrid) {
  __shared__ double sh[24];
  double v[6];
  bn_lc_sums(lc_ptr, lc_row, lc_ent, h, y, keep, mpad, vgrid, v, sh);
  if (threadIdx.x == 0) {
    const int j = lcols[blockIdx.x];
    if constexpr (CP) {
      const f64x2 t = *reinterpret_cast<const f64x2*>(vec + (size_t)j * 2);
      const double vv = t.x, qv = qe[j];
      out[j] = (t.y - v[1]) - qv * v[0] + 2.0 * sigma * v[0] + rho * (v[2] + hc[j] * vv) + eta * vv - v[3] * gsm[j];
    } else {
      const double vv = vec[j], qv = qe[j];
      out[j] = (qv * vv - v[1]) - qv * v[0] + 2.0 * sigma * v[0] + rho * (v[2] + hc[j] * vv) + eta * vv - v[3] * gsm[j];
    }
  }
}

}  // namespace fpsq

// ---- host side

// What a model with coupling terms (fpsq_band_nlp_create_coupled) holds besides fpsq_band_nlp_s' own arrays: the lists of
// fpsq_coupled.h on the device -- partner lists of the stored and of the transposed entries, the latter's own columns, the
// contributor lists of S -- and the values of Wo(q2), Wo(c) on S.  S itself, -Wo(ys) and the n-vector tv (p2 resp. Ptv) are the
// `lin` view's r_rowptr / r_colind / r_vals / tv.  The buffers are on the model's list.
struct bn_terms_s {
  int32_t *pptr = nullptr, *pcol = nullptr, *tpptr = nullptr, *tpcol = nullptr, *tcol = nullptr;
  double *pw = nullptr, *tpw = nullptr;
  int32_t *cptr = nullptr, *crow = nullptr;
  double *cw = nullptr, *wq2 = nullptr, *wc = nullptr;
  int64_t snz = 0;  // value slots: the entries of S, the long rows' behind those of the CSR
  // fpsq_band_nlp_create_coupled_arrow on a handle with long columns: their rows of S, listed apart (fpsq_band.hip.h "LONG
  // ROWS"; lr.cols = 0: none, every row of S is in the CSR)
  int32_t* lrp = nullptr;
  bq_long_rows lr;
};

// fpsq_band_nlp_create: the model's vectors and its two value arrays in the stored row order (a, h: through vperm) and in the
// transposed order (ta, th: through t_perm), gathered once; the three n-vectors an objgrad leaves for the Hessian products;
// `lin`: the view fpsq_band_qp's unchanged kernels take for hprod Val(2) (q = qe).  It borrows the handle's buffers as
// fpsq_band_qp_s does.
struct fpsq_band_nlp_s {
  fpsq_band b = nullptr;
  bool coupled = false;  // the model has coupling terms: `cp` is filled and the launches take their CP forms
  bn_terms_s cp;
  double *q = nullptr, *d = nullptr, *bp = nullptr;  // n, n, m (b in the STORED row order)
  double *a = nullptr, *h = nullptr, *ta = nullptr, *th = nullptr;  // nnz (+ the virtual entries' slot), t_nnz
  double *qe = nullptr, *hc = nullptr, *gs = nullptr;               // q - H'ys, H'c, gs of the last successful objgrad
  // fpsq_band_nlp_create_fn with a code other than 0: the code bytes in both orders (the virtual entries' slot holds 0), and what
  // every objgrad rewrites -- g = G(x) and tg, its transposed order, which the kernels get where the other models hand them
  // h / th (curv() / tcurv()), rem (k_bn_vals_fn) -- and the word a non-finite J(x) raises
  bool fn = false;
  uint8_t *code = nullptr, *tcode = nullptr;
  double *g = nullptr, *tg = nullptr, *rem = nullptr;
  int32_t* flag = nullptr;
  const double* curv() const { return fn ? g : h; }
  const double* tcurv() const { return fn ? tg : th; }
  // fpsq_band_nlp_set_objective_terms: the weights and code bytes per variable, the effective vectors and the partials of f
  // that k_bn_objfn rewrites per objgrad (gridP doubles); `objfn` is off until terms are set and after they are removed, and
  // then every launch takes q and d themselves.  `flag` is allocated with the first terms where the model has none
  bool objfn = false;
  double *ow = nullptr, *qx = nullptr, *de = nullptr, *partO = nullptr;
  uint8_t* ocode = nullptr;
  const double* oq() const { return objfn ? qx : q; }
  const double* od() const { return objfn ? de : d; }
  double *partP = nullptr, *partE = nullptr;
  fpsq_band_qp_s lin;
  uint64_t fact_gen = 0;   // the handle's factorisation count when that objgrad ended
  bool evaluated = false;  // an objgrad has succeeded
  std::vector<void*> allocs;
};

extern "C" {

int fpsq_band_nlp_destroy(fpsq_band_nlp nlp) {
  if (!nlp) return FPSQ_ERR_ARG;
  for (void* p : nlp->allocs) hipFree(p);
  delete nlp;
  return FPSQ_OK;
}

}  // extern "C"

namespace {
// the grid of a kernel that gives a thread an entry (k_bn_vals, k_bcn_vals, k_bcn_assemble, k_gather_d): 256 entries a
// workgroup, capped; above the cap a workgroup walks on
dim3 flat_grid(int64_t len) { return dim3((unsigned)std::max<int64_t>(std::min<int64_t>((len + 255) / 256, 4096), 1)); }

// What the three create entries share: their checks (`entry` names the caller in a refusal; `arrow`: border rows and long
// columns are taken) and the model.  With long columns the transposed arrays span t_nnz entries and gather a slot behind the
// stored values (a = 1, h = 0) into the virtual ones; without them t_nnz = nnz and every size, lane group and launch is what
// it was before the handle's kind was looked at.
int band_nlp_make(const char* entry, bool arrow, fpsq_band b, const double* qdiag, const double* d, const double* bvec,
                  const double* a_vals, const double* h_vals, fpsq_band_nlp* out) {
  if (!b || !qdiag || !d || !bvec || !out || (b->nnz > 0 && (!a_vals || !h_vals))) return FPSQ_ERR_ARG;
  const char* why =
      !arrow && b->border > 0 ? "the handle has border rows"
      : !arrow && b->cols > 0 ? "the handle has long columns (they change the transposed structure)"
      : b->coo_nnz >= 0       ? "the handle was created by a fpsq_band_create_coo entry (its callers do not know the slot order)"
                              : nullptr;
  if (why) {
    b->err = std::string(entry) + ": " + why;
    return FPSQ_ERR_STATE;
  }
  hipSetDevice(b->device);
  if (!b->scal) {  // the scalars of a call: device side and pinned host side
    if (dalloc(b, &b->scal, 8)) return FPSQ_ERR_HIP;
    CHK(b, hipHostMalloc((void**)&b->scal_host, 64, hipHostMallocDefault));
  }
  if (int rc = wait_input(b)) return rc;  // (device-resident values produced on the registered stream)
  std::vector<double> bh((size_t)b->m), bs((size_t)b->m);
  CHK(b, hipMemcpy(bh.data(), bvec, (size_t)b->m * 8, hipMemcpyDefault));
  for (int64_t p = 0; p < b->m; ++p) bs[p] = bh[b->reordered ? b->rperm_host[p] : p];
  fpsq_band_nlp nlp = new fpsq_band_nlp_s();
  nlp->b = b;
  fpsq_band_qp_s& lin = nlp->lin;
  lin.b = b;
  lin.lgA = lane_group(b->nnz, b->m);
  lin.lgT = lane_group(b->t_nnz, b->n);
  lin.gridP = bq_grid(b->mpad, lin.lgA);
  lin.gridE = bq_grid(b->n, lin.lgT);
  const size_t nb8 = (size_t)b->n * 8, mb8 = (size_t)b->m * 8;
  const size_t zb8 = (size_t)(std::max<int64_t>(b->nnz, 1) + (b->cols ? 1 : 0)) * 8, tb8 = (size_t)std::max<int64_t>(b->t_nnz, 1) * 8;
  if (!qp_buffers(nlp, {{(void**)&nlp->q, nb8, qdiag, hipMemcpyDefault},
                        {(void**)&nlp->d, nb8, d, hipMemcpyDefault},
                        {(void**)&nlp->bp, mb8, bs.data(), hipMemcpyHostToDevice},
                        {(void**)&nlp->a, zb8, nullptr, hipMemcpyDefault},
                        {(void**)&nlp->h, zb8, nullptr, hipMemcpyDefault},
                        {(void**)&nlp->ta, tb8, nullptr, hipMemcpyDefault},
                        {(void**)&nlp->th, tb8, nullptr, hipMemcpyDefault},
                        {(void**)&nlp->qe, nb8, nullptr, hipMemcpyDefault},
                        {(void**)&nlp->hc, nb8, nullptr, hipMemcpyDefault},
                        {(void**)&nlp->gs, nb8, nullptr, hipMemcpyDefault},
                        {(void**)&nlp->partP, (size_t)lin.gridP * 16, nullptr, hipMemcpyDefault},
                        {(void**)&nlp->partE, (size_t)lin.gridE * 16, nullptr, hipMemcpyDefault}})) {
    b->err = "band_nlp_create: cannot allocate or fill the model's vectors";
    fpsq_band_nlp_destroy(nlp);
    return FPSQ_ERR_HIP;
  }
  lin.q = nlp->qe;
  lin.d = nlp->d;
  lin.bp = nlp->bp;
  lin.partP = nlp->partP;
  lin.partE = nlp->partE;
  // the two value arrays into both orders, by the gathers a factorisation uses for its values
  hipStream_t s = b->stream;
  const dim3 gz = flat_grid(b->nnz), gt = flat_grid(b->t_nnz);
  for (int w = 0; w < 2 && b->nnz > 0; ++w) {
    const double* src = w ? h_vals : a_vals;
    double *st = w ? nlp->h : nlp->a, *tr = w ? nlp->th : nlp->ta;
    hipError_t e;
    if (b->cols) {  // the slot the virtual entries gather (nothing is in flight on the array yet)
      const double slot = w ? 0.0 : 1.0;
      if (hipMemcpy(st + b->nnz, &slot, 8, hipMemcpyHostToDevice) != hipSuccess) {
        b->err = "band_nlp_create: cannot read the constraint values";
        fpsq_band_nlp_destroy(nlp);
        return FPSQ_ERR_HIP;
      }
    }
    if (b->reordered) {
      e = hipMemcpyAsync(b->vals_in, src, (size_t)b->nnz * 8, hipMemcpyDefault, s);
      hipLaunchKernelGGL(k_gather_d, gz, dim3(256), 0, s, b->vals_in, b->vperm, st, b->nnz);
    } else {
      e = hipMemcpyAsync(st, src, (size_t)b->nnz * 8, hipMemcpyDefault, s);
    }
    hipLaunchKernelGGL(k_gather_d, gt, dim3(256), 0, s, st, b->t_perm, tr, b->t_nnz);
    if (e != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
      b->err = "band_nlp_create: cannot read the constraint values";
      fpsq_band_nlp_destroy(nlp);
      return FPSQ_ERR_HIP;
    }
  }
  *out = nlp;
  return FPSQ_OK;
}

// The term lists of a model that band_nlp_make has made (fpsq_coupled.h builds them on the host from the handle's structure)
int band_nlp_attach(const char* entry, fpsq_band b, fpsq_band_nlp nlp, int64_t nterms, const int32_t* t_row, const int32_t* t_j, const int32_t* t_k,
                    const double* t_w) {
  const size_t T = (size_t)nterms, nnz = (size_t)b->nnz, tnz = (size_t)b->t_nnz, n = (size_t)b->n, m = (size_t)b->m;
  std::vector<int32_t> row(T), cj(T), ck(T), rp(m + 1), ci(std::max<size_t>(nnz, 1)), tperm(std::max<size_t>(tnz, 1));
  std::vector<double> w(T);
  CHK(b, hipMemcpy(row.data(), t_row, T * 4, hipMemcpyDefault));
  CHK(b, hipMemcpy(cj.data(), t_j, T * 4, hipMemcpyDefault));
  CHK(b, hipMemcpy(ck.data(), t_k, T * 4, hipMemcpyDefault));
  CHK(b, hipMemcpy(w.data(), t_w, T * 8, hipMemcpyDefault));
  CHK(b, hipMemcpy(rp.data(), b->rowptr, (m + 1) * 4, hipMemcpyDeviceToHost));
  if (nnz) CHK(b, hipMemcpy(ci.data(), b->colind, nnz * 4, hipMemcpyDeviceToHost));
  if (tnz) CHK(b, hipMemcpy(tperm.data(), b->t_perm, tnz * 4, hipMemcpyDeviceToHost));
  std::vector<int32_t> rinv;
  if (b->reordered) {
    rinv.resize(m);
    for (size_t p = 0; p < m; ++p) rinv[b->rperm_host[p]] = (int32_t)p;
  }
  // the long columns' rows of S apart from the CSR, unless FPSQ_BAND_NLP_LONG_ROWS=0 leaves them to the lane-group kernels
  std::vector<int32_t> lcols;
  bool split = b->cols > 0;
  if (const char* ev = std::getenv("FPSQ_BAND_NLP_LONG_ROWS")) split = split && std::atoi(ev) != 0;
  if (split) {
    lcols.resize((size_t)b->cols);
    CHK(b, hipMemcpy(lcols.data(), b->lc_cols, lcols.size() * 4, hipMemcpyDeviceToHost));
  }
  CoupledLists L;
  const std::string what = coupled_build((int64_t)n, (int64_t)m, rp.data(), ci.data(), b->reordered ? rinv.data() : nullptr,
                                         (int64_t)tnz, tperm.data(), nterms, row.data(), cj.data(), ck.data(), w.data(), L,
                                         (int64_t)lcols.size(), lcols.data());
  if (!what.empty()) {
    b->err = std::string(entry) + ": " + what;
    return FPSQ_ERR_ARG;
  }
  bn_terms_s* cp = &nlp->cp;
  nlp->coupled = true;
  fpsq_band_qp_s& lin = nlp->lin;
  const size_t snz = L.sci.size(), s4 = std::max<size_t>(snz, 1) * 4, s8 = std::max<size_t>(snz, 1) * 8;
  cp->snz = (int64_t)snz;
  lin.sparse_q = true;
  lin.lgR = lane_group((int64_t)L.srp[n], (int64_t)n);  // (from the rows the lane groups walk)
  lin.gridR = bq_grid((int64_t)n, lin.lgR);
  const auto H2D = hipMemcpyHostToDevice;
  const size_t tp = L.tpcol.size();  // 2 T, less what lies in long columns (their transposed rows are virtual)
  if (!qp_buffers(nlp, {{(void**)&cp->pptr, (nnz + 1) * 4, L.pptr.data(), H2D},
                        {(void**)&cp->pcol, 2 * T * 4, L.pcol.data(), H2D},
                        {(void**)&cp->pw, 2 * T * 8, L.pw.data(), H2D},
                        {(void**)&cp->tpptr, (tnz + 1) * 4, L.tpptr.data(), H2D},
                        {(void**)&cp->tpcol, std::max<size_t>(tp, 1) * 4, tp ? L.tpcol.data() : nullptr, H2D},
                        {(void**)&cp->tpw, std::max<size_t>(tp, 1) * 8, tp ? L.tpw.data() : nullptr, H2D},
                        {(void**)&cp->tcol, std::max<size_t>(tnz, 1) * 4, tnz ? L.tcol.data() : nullptr, H2D},
                        {(void**)&lin.r_rowptr, (n + 1) * 4, L.srp.data(), H2D},
                        {(void**)&lin.r_colind, s4, L.sci.data(), H2D},
                        {(void**)&cp->cptr, (snz + 1) * 4, L.cptr.data(), H2D},
                        {(void**)&cp->crow, 2 * T * 4, L.crow.data(), H2D},
                        {(void**)&cp->cw, 2 * T * 8, L.cw.data(), H2D},
                        {(void**)&lin.r_vals, s8, nullptr, H2D},
                        {(void**)&cp->wq2, s8, nullptr, H2D},
                        {(void**)&cp->wc, s8, nullptr, H2D},
                        {(void**)&lin.tv, n * 8, nullptr, H2D},
                        {(void**)&lin.partF, (size_t)lin.gridR * 8, nullptr, H2D},
                        {(void**)&cp->lrp, L.lrp.size() * 4, L.lrp.data(), H2D}})) {
    b->err = std::string(entry) + ": cannot allocate or fill the term lists";
    return FPSQ_ERR_HIP;
  }
  if (split) {
    cp->lr.cols = b->cols;
    cp->lr.ptr = cp->lrp;
    cp->lr.col = lin.r_colind;
    cp->lr.lcols = b->lc_cols;
    cp->lr.cptr = cp->cptr;
    cp->lr.crow = cp->crow;
    cp->lr.cw = cp->cw;
    cp->lr.rv = lin.r_vals;
    cp->lr.wq2 = cp->wq2;
    cp->lr.wc = cp->wc;
    lin.long_rows = &cp->lr;
  }
  return FPSQ_OK;
}
}  // namespace

extern "C" {

int fpsq_band_nlp_create(fpsq_band b, const double* qdiag, const double* d, const double* bvec, const double* a_vals,
                         const double* h_vals, fpsq_band_nlp* out) {
  return band_nlp_make("band_nlp_create", false, b, qdiag, d, bvec, a_vals, h_vals, out);
}

int fpsq_band_nlp_create_arrow(fpsq_band b, const double* qdiag, const double* d, const double* bvec, const double* a_vals,
                               const double* h_vals, fpsq_band_nlp* out) {
  return band_nlp_make("band_nlp_create_arrow", true, b, qdiag, d, bvec, a_vals, h_vals, out);
}

int fpsq_band_nlp_create_fn(fpsq_band b, const double* qdiag, const double* d, const double* bvec, const double* a_vals,
                            const double* h_vals, const uint8_t* fn_codes, fpsq_band_nlp* out) {
  static const char* entry = "band_nlp_create_fn";
  if (!b || !out) return FPSQ_ERR_ARG;
  const size_t nnz = (size_t)b->nnz, tnz = (size_t)b->t_nnz;
  std::vector<uint8_t> codes(nnz + 1, 0);  // (the slot behind the stored entries: what the virtual transposed entries gather)
  bool any = false;
  if (fn_codes && nnz > 0 && b->coo_nnz < 0) {
    hipSetDevice(b->device);
    CHK(b, hipMemcpy(codes.data(), fn_codes, nnz, hipMemcpyDefault));
    for (size_t k = 0; k < nnz; ++k) {
      if (codes[k] >= FPSQ_FN_COUNT) {
        b->err = std::string(entry) + ": fn_codes[" + std::to_string(k) + "] = " + std::to_string((int)codes[k]) +
                 " is not a function code (0 .. " + std::to_string(FPSQ_FN_COUNT - 1) + ")";
        return FPSQ_ERR_ARG;
      }
      any = any || codes[k] != 0;
    }
  }
  fpsq_band_nlp nlp = nullptr;
  if (int rc = band_nlp_make(entry, true, b, qdiag, d, bvec, a_vals, h_vals, &nlp)) return rc;
  if (any) {  // (with every code 0 the model IS fpsq_band_nlp_create_arrow's: the same launches, the same bits)
    std::vector<int32_t> perm(std::max(nnz, tnz));
    std::vector<uint8_t> st(codes), tr(std::max<size_t>(tnz, 1), 0);
    bool ok = true;
    if (b->reordered) {
      ok = hipMemcpy(perm.data(), b->vperm, nnz * 4, hipMemcpyDeviceToHost) == hipSuccess;
      for (size_t k = 0; ok && k < nnz; ++k) st[k] = codes[perm[k]];
    }
    ok = ok && hipMemcpy(perm.data(), b->t_perm, tnz * 4, hipMemcpyDeviceToHost) == hipSuccess;
    for (size_t k = 0; ok && k < tnz; ++k) tr[k] = st[perm[k]];
    const auto H2D = hipMemcpyHostToDevice;
    ok = ok && qp_buffers(nlp, {{(void**)&nlp->code, nnz + 1, st.data(), H2D},
                                {(void**)&nlp->tcode, tr.size(), tr.data(), H2D},
                                {(void**)&nlp->g, nnz * 8, nullptr, H2D},
                                {(void**)&nlp->tg, std::max<size_t>(tnz, 1) * 8, nullptr, H2D},
                                {(void**)&nlp->rem, nnz * 8, nullptr, H2D},
                                {(void**)&nlp->flag, 8, nullptr, H2D}});
    if (!ok || hipMemset(nlp->flag, 0, 8) != hipSuccess) {
      b->err = std::string(entry) + ": cannot allocate or fill the function codes";
      fpsq_band_nlp_destroy(nlp);
      return FPSQ_ERR_HIP;
    }
    nlp->fn = true;
  }
  *out = nlp;
  return FPSQ_OK;
}

int fpsq_band_nlp_create_coupled(fpsq_band b, const double* qdiag, const double* d, const double* bvec, const double* a_vals,
                                 const double* h_vals, int64_t nterms, const int32_t* t_row, const int32_t* t_j,
                                 const int32_t* t_k, const double* t_w, fpsq_band_nlp* out) {
  if (nterms < 0 || (nterms > 0 && (!t_row || !t_j || !t_k || !t_w))) return FPSQ_ERR_ARG;
  fpsq_band_nlp nlp = nullptr;
  if (int rc = band_nlp_make("band_nlp_create_coupled", false, b, qdiag, d, bvec, a_vals, h_vals, &nlp)) return rc;
  if (nterms > 0) {  // (without terms the model IS fpsq_band_nlp_create's: the same launches, the same bits)
    if (int rc = band_nlp_attach("band_nlp_create_coupled", b, nlp, nterms, t_row, t_j, t_k, t_w)) {
      fpsq_band_nlp_destroy(nlp);
      return rc;
    }
  }
  *out = nlp;
  return FPSQ_OK;
}

int fpsq_band_nlp_create_coupled_arrow(fpsq_band b, const double* qdiag, const double* d, const double* bvec, const double* a_vals,
                                       const double* h_vals, int64_t nterms, const int32_t* t_row, const int32_t* t_j,
                                       const int32_t* t_k, const double* t_w, fpsq_band_nlp* out) {
  if (nterms < 0 || (nterms > 0 && (!t_row || !t_j || !t_k || !t_w))) return FPSQ_ERR_ARG;
  fpsq_band_nlp nlp = nullptr;
  if (int rc = band_nlp_make("band_nlp_create_coupled_arrow", true, b, qdiag, d, bvec, a_vals, h_vals, &nlp)) return rc;
  if (nterms > 0) {  // (without terms the model IS fpsq_band_nlp_create_arrow's; without border rows and long columns the
                     // lists and launches are fpsq_band_nlp_create_coupled's)
    if (int rc = band_nlp_attach("band_nlp_create_coupled_arrow", b, nlp, nterms, t_row, t_j, t_k, t_w)) {
      fpsq_band_nlp_destroy(nlp);
      return rc;
    }
  }
  *out = nlp;
  return FPSQ_OK;
}

int fpsq_band_nlp_set_objective_terms(fpsq_band b, fpsq_band_nlp nlp, const double* w, const uint8_t* codes) {
  static const char* entry = "band_nlp_set_objective_terms";
  if (!b || !nlp) return FPSQ_ERR_ARG;
  if (nlp->b != b) {
    b->err = std::string(entry) + ": the model was created on another handle";
    return FPSQ_ERR_ARG;
  }
  nlp->evaluated = false;  // (qe, hc and gs are those of another objective: the next objgrad fixes the point again)
  if (!w) {                // without terms the model is the one it was: the launches take q and d themselves
    nlp->objfn = false;
    return FPSQ_OK;
  }
  hipSetDevice(b->device);
  if (int rc = wait_input(b)) return rc;
  // (device-resident arguments are complete, and nothing of an earlier evaluation reads the arrays below any more)
  CHK(b, hipStreamSynchronize(b->stream));
  const size_t n = (size_t)b->n;
  std::vector<double> wh(n);
  std::vector<uint8_t> ch(n, 0);
  CHK(b, hipMemcpy(wh.data(), w, n * 8, hipMemcpyDefault));
  if (codes) CHK(b, hipMemcpy(ch.data(), codes, n, hipMemcpyDefault));
  for (size_t j = 0; j < n; ++j)
    if (wh[j] != 0.0 && ch[j] >= FPSQ_FN_COUNT) {
      b->err = std::string(entry) + ": codes[" + std::to_string(j) + "] = " + std::to_string((int)ch[j]) +
               " is not a function code (0 .. " + std::to_string(FPSQ_FN_COUNT - 1) + ") and w[" + std::to_string(j) + "] is not 0";
      return FPSQ_ERR_ARG;
    }
  const auto H2D = hipMemcpyHostToDevice;
  bool ok = true;
  if (!nlp->partO)  // (the last of the five: a call that failed half-way allocates again)
    ok = qp_buffers(nlp, {{(void**)&nlp->ow, std::max<size_t>(n, 1) * 8, nullptr, H2D},
                          {(void**)&nlp->qx, std::max<size_t>(n, 1) * 8, nullptr, H2D},
                          {(void**)&nlp->de, std::max<size_t>(n, 1) * 8, nullptr, H2D},
                          {(void**)&nlp->ocode, std::max<size_t>(n, 1), nullptr, H2D},
                          {(void**)&nlp->partO, (size_t)nlp->lin.gridP * 8, nullptr, H2D}});
  if (ok && !nlp->flag) ok = qp_buffers(nlp, {{(void**)&nlp->flag, 8, nullptr, H2D}}) && hipMemset(nlp->flag, 0, 8) == hipSuccess;
  ok = ok && hipMemcpy(nlp->ow, wh.data(), n * 8, H2D) == hipSuccess && hipMemcpy(nlp->ocode, ch.data(), n, H2D) == hipSuccess;
  if (!ok) {
    nlp->objfn = false;
    b->err = std::string(entry) + ": cannot allocate or fill the objective terms";
    return FPSQ_ERR_HIP;
  }
  nlp->objfn = true;
  return FPSQ_OK;
}

int fpsq_band_nlp_cons(fpsq_band b, fpsq_band_nlp nlp, const double* x, double* c) {
  if (!b || !nlp || nlp->b != b || !x || !c) return FPSQ_ERR_ARG;
  hipSetDevice(b->device);
  if (int rc = wait_input(b)) return rc;
  const StagedArg ax = staged(b, x, b->in_a, (size_t)b->n);
  if (int rc = stage_in(b, ax)) return rc;
  const StagedArg oc = staged(b, c, b->o_q1, (size_t)b->m);
  const int lg = nlp->lin.lgA;
  const bn_partners pt{nlp->cp.pptr, nlp->cp.pcol, nlp->cp.pw};
  // (one dispatch on the lane group: the separable and the coupled form, or with function terms k_bn_cons_fn in their place)
  WITH_LANE_GROUP(lg, if (!nlp->fn) { WITH_BOOL(nlp->coupled, CP, hipLaunchKernelGGL(
      (k_bn_cons<LG, CP>), dim3(bq_grid(b->m, lg)), dim3(256), 0, b->stream, b->rowptr, b->colind, nlp->a, nlp->h, ax.tile(),
      nlp->bp, b->row_perm(), oc.tile(), (int)b->m, pt)) } else hipLaunchKernelGGL(
      k_bn_cons_fn<LG>, dim3(bq_grid(b->m, lg)), dim3(256), 0, b->stream, b->rowptr, b->colind, nlp->a, nlp->h, nlp->code, ax.tile(),
      nlp->bp, b->row_perm(), oc.tile(), (int)b->m))
  if (int rc = stage_back(b, oc)) return rc;
  CHK(b, hipStreamSynchronize(b->stream));
  return FPSQ_OK;
}

int fpsq_band_nlp_objgrad(fpsq_band b, fpsq_band_nlp nlp, const double* x, double sigma, double rho, double eta, double delta,
                          const double* xk, double* fx, double* gx, double* ys, double* gs, int32_t* info) {
  if (!b || !nlp || nlp->b != b || !x || !fx || !(delta >= 0.0)) return FPSQ_ERR_ARG;
  hipSetDevice(b->device);
  hipStream_t s = b->stream;
  const fpsq_band_qp_s& lin = nlp->lin;
  const bn_terms_s& cp = nlp->cp;
  const bool coupled = nlp->coupled;
  const int n = (int)b->n, m = (int)b->m, mpad = (int)b->mpad;
  nlp->evaluated = false;
  b->factored = false;
  if (int rc = wait_input(b)) return rc;
  rho = rho > 0.0 ? rho : 0.0;  // (the reference adds these terms only when the parameter is positive)
  eta = eta > 0.0 ? eta : 0.0;
  const StagedArg ax = staged(b, x, b->in_a, (size_t)n);
  if (int rc = stage_in(b, ax)) return rc;
  const StagedArg axk = staged(b, eta > 0.0 ? xk : nullptr, b->in_b, (size_t)n);
  if (int rc = stage_in(b, axk)) return rc;
  // 1: J(x) into the handle's value arrays, the stored CSR and the transposed one (with terms: by the same kernel)
  b->have_vals = true;
  if (b->nnz > 0 && coupled) {
    hipLaunchKernelGGL(k_bcn_vals, flat_grid(b->nnz), dim3(256), 0, s, nlp->a, nlp->h, b->colind, cp.pptr, cp.pcol, cp.pw,
                       ax.tile(), b->vals, b->nnz);
    hipLaunchKernelGGL(k_bcn_vals, flat_grid(b->t_nnz), dim3(256), 0, s, nlp->ta, nlp->th, cp.tcol, cp.tpptr, cp.tpcol, cp.tpw,
                       ax.tile(), b->t_vals, b->t_nnz);
    if (b->fb_nnz > 0)  // (as below)
      hipLaunchKernelGGL(k_gather_d, flat_grid(b->fb_nnz), dim3(256), 0, s, b->vals, b->fb_perm, b->fb_vals, b->fb_nnz);
  } else if (b->nnz > 0) {  // (with function terms: the function forms of the two launches, which also write G(x) and rem)
    if (!nlp->fn)
      hipLaunchKernelGGL(k_bn_vals, flat_grid(b->nnz), dim3(256), 0, s, nlp->a, nlp->h, b->colind, ax.tile(), b->vals, b->nnz);
    else
      hipLaunchKernelGGL(k_bn_vals_fn, flat_grid(b->nnz), dim3(256), 0, s, nlp->a, nlp->h, nlp->code, b->colind, ax.tile(), b->vals,
                         nlp->g, nlp->rem, nlp->flag, b->nnz);
    WITH_LANE_GROUP(lin.lgT, if (!nlp->fn) hipLaunchKernelGGL(k_bn_tvals<LG>, dim3(lin.gridE), dim3(256), 0, s, b->t_rowptr, nlp->ta,
                                                              nlp->th, ax.tile(), b->t_vals, n);
                    else hipLaunchKernelGGL(k_bn_tvals_fn<LG>, dim3(lin.gridE), dim3(256), 0, s, b->t_rowptr, nlp->ta, nlp->th,
                                            nlp->tcode, ax.tile(), b->t_vals, nlp->tg, n))
    if (b->fb_nnz > 0)  // (long columns and k_band_form: the values of the other columns alone, as fpsq_band_factorize)
      hipLaunchKernelGGL(k_gather_d, flat_grid(b->fb_nnz), dim3(256), 0, s, b->vals, b->fb_perm, b->fb_vals, b->fb_nnz);
  }
  // with function terms in the objective: the effective (q, d) of this x and the partials of f, behind the value launches
  const double *oq = nlp->oq(), *od = nlp->od();
  if (nlp->objfn)
    hipLaunchKernelGGL(k_bn_objfn, dim3(lin.gridP), dim3(256), 0, s, ax.tile(), nlp->q, nlp->d, nlp->ow, nlp->ocode, nlp->qx, nlp->de,
                       nlp->partO, nlp->flag, n);
  if (nlp->fn || nlp->objfn) {  // a non-finite J(x) or objective term must not reach the factorisation: what a failed one
                                // returns, before one is enqueued (one word: 1 = J(x), 2 = the objective)
    int32_t* raised = reinterpret_cast<int32_t*>(b->scal_host + 7);  // (pinned; the scalars of a call end at [4])
    CHK(b, hipMemcpyAsync(raised, nlp->flag, 4, hipMemcpyDeviceToHost, s));
    CHK(b, hipStreamSynchronize(s));
    if (*raised) {
      CHK(b, hipMemsetAsync(nlp->flag, 0, 4, s));
      b->err = std::string("band_nlp_objgrad: ") +
               (*raised == 1   ? "J(x) holds"
                : *raised == 2 ? "the objective's function terms hold"
                               : "J(x) and the objective's function terms hold") +
               " a non-finite value (nothing was factorised or evaluated)";
      *fx = std::numeric_limits<double>::quiet_NaN();
      if (info) *info = -1;
      return 1;
    }
  }
  // 2: the numeric factorisation on them
  if (int rc = band_factor_numeric(b, delta, info)) return rc;  // (1: no valid factor, *info says where; nothing is evaluated)
  // 3 - 5: the evaluation on that factor
  if (int rc = eval_begin(b)) return rc;
  const StagedArg ogx = staged(b, gx, b->o_p1, (size_t)n), ogs = staged(b, gs, b->o_p2, (size_t)n),
                  oys = staged(b, ys, b->o_q1, (size_t)m);
  double* keep = b->cols ? b->bd_keep : b->o_q2;  // (long columns: the operand has virtual rows, as in bq_launches)
  hipLaunchKernelGGL(k_bq_pack<false>, grid256(n), dim3(256), 0, s, ax.tile(), oq, od, b->xn, n);
  WITH_LANE_GROUP(lin.lgA, if (!nlp->fn) { WITH_BOOL(coupled, CP, hipLaunchKernelGGL(
      (k_bn_prologue<LG, CP>), dim3(lin.gridP), dim3(256), 0, s, b->rowptr, b->colind, b->vals, CP ? nlp->a : nlp->h, b->xn,
      ax.tile(), oq, od, nlp->bp, b->r2, keep, nlp->partP, m, mpad, n)) } else hipLaunchKernelGGL(
      (k_bn_prologue<LG, false, true>), dim3(lin.gridP), dim3(256), 0, s, b->rowptr, b->colind, b->vals, nlp->rem, b->xn,
      ax.tile(), oq, od, nlp->bp, b->r2, keep, nlp->partP, m, mpad, n))
  if (b->cols) cols_keep<1>(b, keep);
  band_solve(b);
  WITH_LANE_GROUP(lin.lgT, WITH_BOOL(coupled, CP, hipLaunchKernelGGL(
      (k_bn_epilogue<LG, CP>), dim3(lin.gridE), dim3(256), 0, s, b->t_rowptr, b->t_colind, b->t_vals, nlp->tcurv(), b->r2, keep,
      b->row_perm(), ax.tile(), axk.tile(), oq, od, sigma, rho, eta, ogx.tile(), ogs.tile(), oys.tile(), nlp->qe, nlp->hc,
      nlp->gs, lin.tv, nlp->partE, n, m)))
  if (b->cols)  // the curvature sums at the long columns, whose transposed rows are virtual
    hipLaunchKernelGGL(k_bn_lc_epilogue, dim3(b->cols), dim3(256), 0, s, b->lc_ptr, b->lc_row, b->lc_ent, b->lc_cols, nlp->curv(),
                       b->r2, keep, ax.tile(), axk.tile(), oq, nlp->gs, sigma, rho, eta, ogx.tile(), nlp->qe, nlp->hc, mpad,
                       b->bc_grid);
  if (coupled) {  // the values of Wo on S, then the rows of S that gx lacks
    hipLaunchKernelGGL(k_bcn_assemble, flat_grid(cp.snz), dim3(256), 0, s, cp.cptr, cp.crow, cp.cw, b->r2, keep, sigma,
                       lin.r_vals, cp.wq2, cp.wc, cp.snz);
    if (gx)
      WITH_LANE_GROUP(lin.lgR, hipLaunchKernelGGL(k_bcn_finish<LG>, dim3(lin.gridR), dim3(256), 0, s, lin.r_rowptr, lin.r_colind,
                                                  lin.r_vals, cp.wq2, lin.tv, nlp->gs, ogx.tile(), n))
    if (gx && cp.lr.cols)  // the long columns' rows of S (k_bn_lc_epilogue has rewritten gx there)
      hipLaunchKernelGGL(k_bq_long_rows<LR_OBJ>, dim3(cp.lr.cols), dim3(256), 0, s, cp.lr, (const double*)nlp->gs,
                         (const double*)lin.tv, (const double*)nullptr, (const double*)nullptr, 0.0, ogx.tile());
  }
  if (nlp->objfn)  // (f from k_bn_objfn's partials; the prologue's own slice, formed from the effective vectors, is not read)
    hipLaunchKernelGGL(k_bq_phi_sq, dim3(1), dim3(256), 0, s, nlp->partO, lin.gridP, nlp->partP, lin.gridP, nlp->partE, lin.gridE,
                       rho, eta, b->scal);
  else
    hipLaunchKernelGGL(k_bq_phi, dim3(1), dim3(256), 0, s, nlp->partP, lin.gridP, nlp->partE, lin.gridE, rho, eta, b->scal);
  for (const StagedArg* o : {&ogx, &ogs, &oys})
    if (int rc = stage_back(b, *o)) return rc;
  if (int rc = eval_end(b, 5, &b->info.last_solve_ms)) return rc;
  *fx = b->scal_host[0];
  nlp->fact_gen = b->fact_gen;
  nlp->evaluated = true;
  return FPSQ_OK;
}

int fpsq_band_nlp_hprod(fpsq_band b, fpsq_band_nlp nlp, const double* v, double sigma, double rho, double eta,
                        int32_t hessian_approx, double* Hv) {
  if (!b || !nlp || nlp->b != b || !v || !Hv) return FPSQ_ERR_ARG;
  if (hessian_approx != 1 && hessian_approx != 2) {
    b->err = "band_nlp_hprod: hessian_approx must be 1 or 2";
    return FPSQ_ERR_ARG;
  }
  if (!nlp->evaluated) {
    b->err = "band_nlp_hprod: no successful fpsq_band_nlp_objgrad of this model yet (it fixes the point of the product)";
    return FPSQ_ERR_STATE;
  }
  if (nlp->fact_gen != b->fact_gen) {
    b->err = "band_nlp_hprod: the handle was factorised again since this model's last objgrad (its values are no longer J(x))";
    return FPSQ_ERR_STATE;
  }
  if (int rc = eval_begin(b)) return rc;
  hipStream_t s = b->stream;
  fpsq_band_qp_s& lin = nlp->lin;
  const bn_terms_s& cp = nlp->cp;
  const bool coupled = nlp->coupled;
  const int n = (int)b->n, m = (int)b->m, mpad = (int)b->mpad;
  rho = rho > 0.0 ? rho : 0.0;
  eta = eta > 0.0 ? eta : 0.0;
  const StagedArg av = staged(b, v, b->in_a, (size_t)n);
  if (int rc = stage_in(b, av)) return rc;
  const StagedArg ah = staged(b, Hv, b->o_p1, (size_t)n);
  if (hessian_approx == 2) {
    // the linear model's launches with q = qe (with terms: their sparse form, Q = diag(qe) - Wo(ys)), then the curvature of
    // rho/2 |c|^2
    bq_launches(b, &lin, true, av.tile(), nullptr, sigma, rho, eta, ah.tile(), nullptr, nullptr);
    if (rho > 0.0 && coupled)
      WITH_LANE_GROUP(lin.lgR, hipLaunchKernelGGL(k_bcn_hcv<LG>, dim3(lin.gridR), dim3(256), 0, s, lin.r_rowptr, lin.r_colind,
                                                  cp.wc, nlp->hc, av.tile(), ah.tile(), n))
    else if (rho > 0.0)
      hipLaunchKernelGGL(k_bn_hcv, grid256(n), dim3(256), 0, s, nlp->hc, av.tile(), ah.tile(), n);
  } else {
    double* keep = b->cols ? b->bd_keep : b->o_q2;
    if (coupled) {  // xn[j] = {v_j, (E v)_j}, E = diag(qe) - Wo(ys)
      WITH_LANE_GROUP(lin.lgR, hipLaunchKernelGGL((k_bq_pack_sq<LG, true>), dim3(lin.gridR), dim3(256), 0, s, lin.r_rowptr,
                                                  lin.r_colind, lin.r_vals, av.tile(), nlp->qe, nlp->d, b->xn, lin.partF, n))
      if (cp.lr.cols)
        hipLaunchKernelGGL(k_bq_long_rows<LR_PACK>, dim3(cp.lr.cols), dim3(256), 0, s, cp.lr, av.tile(), (const double*)nullptr,
                           (const double*)nullptr, (const double*)nullptr, 0.0, b->xn);
    } else
      hipLaunchKernelGGL(k_bq_pack<true>, grid256(n), dim3(256), 0, s, av.tile(), nlp->qe, nlp->d, b->xn, n);
    WITH_LANE_GROUP(lin.lgA, hipLaunchKernelGGL((k_bq_prologue<LG, true, false>), dim3(lin.gridP), dim3(256), 0, s, b->rowptr,
                                                b->colind, b->vals, b->xn, av.tile(), nlp->qe, nlp->d, nlp->bp, b->r2, keep,
                                                nlp->partP, m, mpad, n))
    if (b->cols) cols_keep<1>(b, keep);
    band_solve(b);
    WITH_LANE_GROUP(lin.lgT, WITH_BOOL(coupled, CP, hipLaunchKernelGGL(
        (k_bn_epilogue_h1<LG, CP>), dim3(lin.gridE), dim3(256), 0, s, b->t_rowptr, b->t_colind, b->t_vals, nlp->tcurv(), b->r2, keep,
        CP ? b->xn : av.tile(), nlp->qe, nlp->hc, nlp->gs, sigma, rho, eta, ah.tile(), lin.tv, n)))
    if (b->cols) {  // (H'q1)_j at the long columns, before the second solve takes b->r2
      WITH_BOOL(coupled, CP, hipLaunchKernelGGL(k_bn_lc_epilogue_h1<CP>, dim3(b->cols), dim3(256), 0, s, b->lc_ptr, b->lc_row,
                                                b->lc_ent, b->lc_cols, nlp->curv(), b->r2, keep, CP ? b->xn : av.tile(), nlp->qe,
                                                nlp->hc, nlp->gs, sigma, rho, eta, ah.tile(), mpad, b->bc_grid))
    }
    if (coupled) {  // the rows of S, while b->r2 still holds the first solve
      WITH_LANE_GROUP(lin.lgR, hipLaunchKernelGGL(k_bcn_finish_h1<LG>, dim3(lin.gridR), dim3(256), 0, s, lin.r_rowptr,
                                                  lin.r_colind, cp.cptr, cp.crow, cp.cw, lin.r_vals, cp.wc, b->r2, lin.tv,
                                                  av.tile(), nlp->gs, rho, ah.tile(), n))
      if (cp.lr.cols)
        hipLaunchKernelGGL(k_bq_long_rows<LR_HV1>, dim3(cp.lr.cols), dim3(256), 0, s, cp.lr, av.tile(), (const double*)lin.tv,
                           (const double*)nlp->gs, (const double*)b->r2, rho, ah.tile());
    }
    // z = M^-1 ghjvprod(x, gs, v) = M^-1 H (gs .* v) [+ the terms] on the cached factor (tau = delta, include/fpsq.h), Hv -= J'z
    const bn_partners pt{cp.pptr, cp.pcol, cp.pw};
    WITH_LANE_GROUP(lin.lgA, WITH_BOOL(coupled, CP, hipLaunchKernelGGL(
        (k_bn_hgv<LG, CP>), dim3(lin.gridP), dim3(256), 0, s, b->rowptr, b->colind, nlp->curv(), nlp->gs, av.tile(), b->r2, m, mpad,
        pt)))
    band_solve(b);
    WITH_LANE_GROUP(lin.lgT, hipLaunchKernelGGL(k_bn_jtz<LG>, dim3(lin.gridE), dim3(256), 0, s, b->t_rowptr, b->t_colind,
                                                b->t_vals, b->r2, ah.tile(), n))
  }
  if (int rc = stage_back(b, ah)) return rc;
  return eval_end(b, 0, &b->info.last_solve_ms);
}
}  // extern "C"
