// fpsq_band_cnlp.hip.h -- part of the fpsq_band.hip translation unit (included behind fpsq_band_nlp.hip.h): COUPLED quadratic
// constraints on the device-resident nonlinear model (C ABI: include/fpsq.h, fpsq_band_nlp_create_coupled),
//   c_i(x) = sum_j (A_ij + 1/2 H_ij x_j) x_j + sum_{t in i} w_t x_jt x_kt - b_i,    jt != kt both columns of row i of A,
// so J(x)_ij = A_ij + H_ij x_j + sum w_t x_partner keeps the handle's pattern, sum_i y_i Hess c_i = diag(H'y) + Wo(y) with
// Wo(y) sparse symmetric on a pattern S fixed at create, and ghjvprod gains w_t (g_j v_k + g_k v_j).  The index lists come from
// fpsq_coupled.h.  The model's `lin` view carries S and -Wo(ys) as the R of a sparse objective Hessian, so hprod Val(2) is
// bq_launches' sparse form with Q = diag(qe) - Wo(ys), unchanged.  The kernels follow k_bn_*: a lane group per row, grid-stride
// tiles, sums in a fixed order (a lane's entries in index order, lanes by xor shuffles, workgroups in index order), no
// floating-point atomics.  None of k_bn_* / k_bq_* is edited: a model without terms runs fpsq_band_nlp.hip.h's launches.
#pragma once
#include "fpsq_coupled.h"

namespace fpsq {

// vals[k] = a[k] + h[k] x[col[k]] + sum_u pw[u] x[pcol[u]] over the entries of ONE CSR and their partner lists: launched on the
// stored structure (col = colind) and on the transposed one (col = the entry's own column, its lists in the same order), so
// both value arrays get the same bits
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

// k_bn_prologue for a symmetric curvature of any kind: c_p = sum 1/2 (J + a) x_c - b_p, which needs no walk of the term lists
// (J = vals already holds them).  Everything else as there.
template <int LG>
__global__ __launch_bounds__(256) void k_bcn_prologue(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                      const double* __restrict__ vals, const double* __restrict__ a,
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
        const double jv = vals[k], av = a[k];
        const f64x2 t = *reinterpret_cast<const f64x2*>(xg + (size_t)colind[k] * 2);
        a0 += jv * t.x;
        a1 += (0.5 * (jv + av)) * t.y;
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

// c(x) alone from the model's own arrays, in the caller's row order: c_p = sum (a + 1/2 h x_c + 1/2 sum_u pw x_partner) x_c - b_p
// (every term is met at both of its entries, half each)
template <int LG>
__global__ __launch_bounds__(256) void k_bcn_cons(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                  const double* __restrict__ a, const double* __restrict__ h,
                                                  const int32_t* __restrict__ pptr, const int32_t* __restrict__ pcol,
                                                  const double* __restrict__ pw, const double* __restrict__ x,
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
        double ps = 0.0;
        const int ue = pptr[k + 1];
        for (int u = pptr[k]; u < ue; ++u) ps += pw[u] * x[pcol[u]];
        s += (a[k] + 0.5 * h[k] * xv + 0.5 * ps) * xv;
      }
    }
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (l == 0 && p < m) c[rperm ? rperm[p] : p] = s - bp[p];
  }
}

// k_bn_epilogue that also leaves p2_j = -s2 in tv for the finish launch.  Its gx_j lacks Wo(ys) p2 + Wo(q2) gs, whose rows need
// every p2 and gs: k_bcn_finish adds them.
template <int LG>
__global__ __launch_bounds__(256) void k_bcn_epilogue(const int32_t* __restrict__ t_rowptr, const int32_t* __restrict__ t_colind,
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
      tv[j] = p2;
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

// The values of -Wo(ys), Wo(q2), Wo(c) on S in one pass over the contributor lists (increasing stored row): y[p] = {q1, q2} the
// sweeps' solution, keep = c, ys_p = q1 + sigma q2 as the epilogue forms it.  rv = -Wo(ys) is the R of the model's `lin` view.
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

// hprod Val(2), behind bq_launches' sparse form (Q = diag(qe) - Wo(ys)): Hv_j += hc_j v_j + (Wo(c) v)_j   (not scaled by rho)
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

// k_bn_epilogue_h1 with E = diag(qe) - Wo(ys) in the place of qe: xg[j] = {v_j, (E v)_j} is what k_bq_pack_sq<HP> packed (the
// second solve's right-hand side was J (E v)); the row's own terms as there, Ptv_j = s1 is left in tv for k_bcn_finish_h1
template <int LG>
__global__ __launch_bounds__(256) void k_bcn_epilogue_h1(const int32_t* __restrict__ t_rowptr, const int32_t* __restrict__ t_colind,
                                                         const double* __restrict__ t_vals, const double* __restrict__ th,
                                                         const double* __restrict__ y, const double* __restrict__ keep,
                                                         const double* __restrict__ xg, const double* __restrict__ qe,
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
      const f64x2 t = *reinterpret_cast<const f64x2*>(xg + (size_t)j * 2);
      const double vv = t.x, qv = qe[j];
      out[j] = (t.y - s2) - qv * s1 + 2.0 * sigma * s1 + rho * (s3 + hc[j] * vv) + eta * vv - h1 * gsm[j];
      tv[j] = s1;
    }
  }
}

// hprod Val(1), the rows of S: Hv_j += sum_k (Wo(ys)_jk Ptv_k + rho Wo(c)_jk v_k - Wo(q1)_jk gs_k).  Wo(q1) is used once, so
// its entries are summed here from the contributor lists and the first solve's y[p] = {q1, .} (before the second solve takes y)
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

// Ssv = ghjvprod(x, gs, v) with the terms, into the sweeps' right-hand-side layout r[p] = {Ssv_p, 0} (zero on the padding):
// Ssv_p = sum_k gs_c (h_k v_c + sum_u pw v_partner)
template <int LG>
__global__ __launch_bounds__(256) void k_bcn_hgv(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                 const double* __restrict__ h, const int32_t* __restrict__ pptr,
                                                 const int32_t* __restrict__ pcol, const double* __restrict__ pw,
                                                 const double* __restrict__ gsm, const double* __restrict__ v,
                                                 double* __restrict__ r, int m, int mpad) {
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
        double t = h[k] * v[c];
        const int ue = pptr[k + 1];
        for (int u = pptr[k]; u < ue; ++u) t += pw[u] * v[pcol[u]];
        s += gsm[c] * t;
      }
    }
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (l == 0 && p < mpad) *reinterpret_cast<f64x2*>(r + (size_t)p * 2) = f64x2{s, 0.0};
  }
}

}  // namespace fpsq

// ---- host side

namespace {

dim3 flat_grid(int64_t len) { return dim3((unsigned)std::max<int64_t>(std::min<int64_t>((len + 255) / 256, 4096), 1)); }

int band_cnlp_attach(fpsq_band b, fpsq_band_nlp nlp, int64_t nterms, const int32_t* t_row, const int32_t* t_j, const int32_t* t_k,
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
  CoupledLists L;
  const std::string what = coupled_build((int64_t)n, (int64_t)m, rp.data(), ci.data(), b->reordered ? rinv.data() : nullptr,
                                         (int64_t)tnz, tperm.data(), nterms, row.data(), cj.data(), ck.data(), w.data(), L);
  if (!what.empty()) {
    b->err = "band_nlp_create_coupled: " + what;
    return FPSQ_ERR_ARG;
  }
  fpsq_band_cnlp_s* cp = new fpsq_band_cnlp_s();
  nlp->cp = cp;
  fpsq_band_qp_s& lin = nlp->lin;
  const size_t snz = L.sci.size(), s4 = std::max<size_t>(snz, 1) * 4, s8 = std::max<size_t>(snz, 1) * 8;
  cp->snz = (int64_t)snz;
  lin.sparse_q = true;
  lin.lgR = lane_group((int64_t)snz, (int64_t)n);
  lin.gridR = bq_grid((int64_t)n, lin.lgR);
  const auto H2D = hipMemcpyHostToDevice;
  if (!qp_buffers(nlp, {{(void**)&cp->pptr, (nnz + 1) * 4, L.pptr.data(), H2D},
                        {(void**)&cp->pcol, 2 * T * 4, L.pcol.data(), H2D},
                        {(void**)&cp->pw, 2 * T * 8, L.pw.data(), H2D},
                        {(void**)&cp->tpptr, (tnz + 1) * 4, L.tpptr.data(), H2D},
                        {(void**)&cp->tpcol, 2 * T * 4, L.tpcol.data(), H2D},
                        {(void**)&cp->tpw, 2 * T * 8, L.tpw.data(), H2D},
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
                        {(void**)&lin.partF, (size_t)lin.gridR * 8, nullptr, H2D}})) {
    b->err = "band_nlp_create_coupled: cannot allocate or fill the term lists";
    return FPSQ_ERR_HIP;
  }
  return FPSQ_OK;
}

int band_cnlp_cons(fpsq_band b, fpsq_band_nlp nlp, const double* x, double* c) {
  const fpsq_band_cnlp_s* cp = nlp->cp;
  hipSetDevice(b->device);
  if (int rc = wait_input(b)) return rc;
  const StagedArg ax = staged(b, x, b->in_a, (size_t)b->n);
  if (int rc = stage_in(b, ax)) return rc;
  const StagedArg oc = staged(b, c, b->o_q1, (size_t)b->m);
  const int lg = nlp->lin.lgA;
  WITH_LANE_GROUP(lg, hipLaunchKernelGGL(k_bcn_cons<LG>, dim3(bq_grid(b->m, lg)), dim3(256), 0, b->stream, b->rowptr, b->colind,
                                         nlp->a, nlp->h, cp->pptr, cp->pcol, cp->pw, ax.tile(), nlp->bp, b->row_perm(), oc.tile(),
                                         (int)b->m))
  if (int rc = stage_back(b, oc)) return rc;
  CHK(b, hipStreamSynchronize(b->stream));
  return FPSQ_OK;
}

// fpsq_band_nlp_objgrad's steps with the terms: launches vals, vals (transposed), [factorisation], pack, prologue, [the sweeps],
// epilogue, assemble, finish, phi
int band_cnlp_objgrad(fpsq_band b, fpsq_band_nlp nlp, const double* x, double sigma, double rho, double eta, double delta,
                      const double* xk, double* fx, double* gx, double* ys, double* gs, int32_t* info) {
  const fpsq_band_cnlp_s* cp = nlp->cp;
  hipSetDevice(b->device);
  hipStream_t s = b->stream;
  const fpsq_band_qp_s& lin = nlp->lin;
  const int n = (int)b->n, m = (int)b->m, mpad = (int)b->mpad;
  nlp->evaluated = false;
  b->factored = false;
  if (int rc = wait_input(b)) return rc;
  rho = rho > 0.0 ? rho : 0.0;
  eta = eta > 0.0 ? eta : 0.0;
  const StagedArg ax = staged(b, x, b->in_a, (size_t)n);
  if (int rc = stage_in(b, ax)) return rc;
  const StagedArg axk = staged(b, eta > 0.0 ? xk : nullptr, b->in_b, (size_t)n);
  if (int rc = stage_in(b, axk)) return rc;
  // 1: J(x) into the handle's value arrays, the stored CSR and the transposed one, by the same kernel
  b->have_vals = true;
  if (b->nnz > 0) {
    hipLaunchKernelGGL(k_bcn_vals, flat_grid(b->nnz), dim3(256), 0, s, nlp->a, nlp->h, b->colind, cp->pptr, cp->pcol, cp->pw,
                       ax.tile(), b->vals, b->nnz);
    hipLaunchKernelGGL(k_bcn_vals, flat_grid(b->t_nnz), dim3(256), 0, s, nlp->ta, nlp->th, cp->tcol, cp->tpptr, cp->tpcol, cp->tpw,
                       ax.tile(), b->t_vals, b->t_nnz);
  }
  // 2: the numeric factorisation on them
  if (int rc = band_factor_numeric(b, delta, info)) return rc;
  // 3 - 5: the evaluation on that factor
  if (int rc = eval_begin(b)) return rc;
  const StagedArg ogx = staged(b, gx, b->o_p1, (size_t)n), ogs = staged(b, gs, b->o_p2, (size_t)n),
                  oys = staged(b, ys, b->o_q1, (size_t)m);
  double* keep = b->o_q2;
  hipLaunchKernelGGL(k_bq_pack<false>, grid256(n), dim3(256), 0, s, ax.tile(), nlp->q, nlp->d, b->xn, n);
  WITH_LANE_GROUP(lin.lgA, hipLaunchKernelGGL(k_bcn_prologue<LG>, dim3(lin.gridP), dim3(256), 0, s, b->rowptr, b->colind, b->vals,
                                              nlp->a, b->xn, ax.tile(), nlp->q, nlp->d, nlp->bp, b->r2, keep, nlp->partP, m, mpad,
                                              n))
  band_solve(b);
  WITH_LANE_GROUP(lin.lgT, hipLaunchKernelGGL(k_bcn_epilogue<LG>, dim3(lin.gridE), dim3(256), 0, s, b->t_rowptr, b->t_colind,
                                              b->t_vals, nlp->th, b->r2, keep, b->row_perm(), ax.tile(), axk.tile(), nlp->q,
                                              nlp->d, sigma, rho, eta, ogx.tile(), ogs.tile(), oys.tile(), nlp->qe, nlp->hc,
                                              nlp->gs, lin.tv, nlp->partE, n, m))
  hipLaunchKernelGGL(k_bcn_assemble, flat_grid(cp->snz), dim3(256), 0, s, cp->cptr, cp->crow, cp->cw, b->r2, keep, sigma,
                     lin.r_vals, cp->wq2, cp->wc, cp->snz);
  if (gx)
    WITH_LANE_GROUP(lin.lgR, hipLaunchKernelGGL(k_bcn_finish<LG>, dim3(lin.gridR), dim3(256), 0, s, lin.r_rowptr, lin.r_colind,
                                                lin.r_vals, cp->wq2, lin.tv, nlp->gs, ogx.tile(), n))
  hipLaunchKernelGGL(k_bq_phi, dim3(1), dim3(256), 0, s, nlp->partP, lin.gridP, nlp->partE, lin.gridE, rho, eta, b->scal);
  for (const StagedArg* o : {&ogx, &ogs, &oys})
    if (int rc = stage_back(b, *o)) return rc;
  if (int rc = eval_end(b, 5, &b->info.last_solve_ms)) return rc;
  *fx = b->scal_host[0];
  nlp->fact_gen = b->fact_gen;
  nlp->evaluated = true;
  return FPSQ_OK;
}

// the launches of an hprod between its staged arguments (fpsq_band_nlp_hprod has checked the state and begun the evaluation).
// Val(2): bq_launches' sparse form (pack_sq, prologue, [sweeps], epilogue_sq, the product with R) [+ k_bcn_hcv when rho > 0].
// Val(1): pack_sq, prologue, [sweeps], epilogue_h1, finish_h1, hgv, [sweeps], jtz.
void band_cnlp_hprod_launches(fpsq_band b, fpsq_band_nlp nlp, const double* v, double sigma, double rho, double eta,
                              int32_t hessian_approx, double* Hv) {
  const fpsq_band_cnlp_s* cp = nlp->cp;
  hipStream_t s = b->stream;
  fpsq_band_qp_s& lin = nlp->lin;
  const int n = (int)b->n, m = (int)b->m, mpad = (int)b->mpad;
  if (hessian_approx == 2) {
    bq_launches(b, &lin, true, v, nullptr, sigma, rho, eta, Hv, nullptr, nullptr);
    if (rho > 0.0)
      WITH_LANE_GROUP(lin.lgR, hipLaunchKernelGGL(k_bcn_hcv<LG>, dim3(lin.gridR), dim3(256), 0, s, lin.r_rowptr, lin.r_colind,
                                                  cp->wc, nlp->hc, v, Hv, n))
    return;
  }
  double* keep = b->o_q2;
  WITH_LANE_GROUP(lin.lgR, hipLaunchKernelGGL((k_bq_pack_sq<LG, true>), dim3(lin.gridR), dim3(256), 0, s, lin.r_rowptr,
                                              lin.r_colind, lin.r_vals, v, nlp->qe, nlp->d, b->xn, lin.partF, n))
  WITH_LANE_GROUP(lin.lgA, hipLaunchKernelGGL((k_bq_prologue<LG, true, false>), dim3(lin.gridP), dim3(256), 0, s, b->rowptr,
                                              b->colind, b->vals, b->xn, v, nlp->qe, nlp->d, nlp->bp, b->r2, keep, nlp->partP, m,
                                              mpad, n))
  band_solve(b);
  WITH_LANE_GROUP(lin.lgT, hipLaunchKernelGGL(k_bcn_epilogue_h1<LG>, dim3(lin.gridE), dim3(256), 0, s, b->t_rowptr, b->t_colind,
                                              b->t_vals, nlp->th, b->r2, keep, b->xn, nlp->qe, nlp->hc, nlp->gs, sigma, rho, eta,
                                              Hv, lin.tv, n))
  WITH_LANE_GROUP(lin.lgR, hipLaunchKernelGGL(k_bcn_finish_h1<LG>, dim3(lin.gridR), dim3(256), 0, s, lin.r_rowptr, lin.r_colind,
                                              cp->cptr, cp->crow, cp->cw, lin.r_vals, cp->wc, b->r2, lin.tv, v, nlp->gs, rho, Hv,
                                              n))
  // z = M^-1 ghjvprod(x, gs, v) on the cached factor, Hv -= J'z
  WITH_LANE_GROUP(lin.lgA, hipLaunchKernelGGL(k_bcn_hgv<LG>, dim3(lin.gridP), dim3(256), 0, s, b->rowptr, b->colind, nlp->h,
                                              cp->pptr, cp->pcol, cp->pw, nlp->gs, v, b->r2, m, mpad))
  band_solve(b);
  WITH_LANE_GROUP(lin.lgT, hipLaunchKernelGGL(k_bn_jtz<LG>, dim3(lin.gridE), dim3(256), 0, s, b->t_rowptr, b->t_colind, b->t_vals,
                                              b->r2, Hv, n))
}
}  // namespace

extern "C" {

int fpsq_band_nlp_create_coupled(fpsq_band b, const double* qdiag, const double* d, const double* bvec, const double* a_vals,
                                 const double* h_vals, int64_t nterms, const int32_t* t_row, const int32_t* t_j,
                                 const int32_t* t_k, const double* t_w, fpsq_band_nlp* out) {
  if (!b || !qdiag || !d || !bvec || !out || (b->nnz > 0 && (!a_vals || !h_vals)) || nterms < 0 ||
      (nterms > 0 && (!t_row || !t_j || !t_k || !t_w)))
    return FPSQ_ERR_ARG;
  const char* why = b->border > 0    ? "the handle has border rows"
                    : b->cols > 0    ? "the handle has long columns (they change the transposed structure)"
                    : b->coo_nnz >= 0 ? kNlpCooRefused
                                      : nullptr;
  if (why) {
    b->err = std::string("band_nlp_create_coupled: ") + why;
    return FPSQ_ERR_STATE;
  }
  fpsq_band_nlp nlp = nullptr;
  if (int rc = band_nlp_make(b, qdiag, d, bvec, a_vals, h_vals, &nlp)) return rc;
  if (nterms > 0) {  // (without terms the model IS fpsq_band_nlp_create's: the same launches, the same bits)
    if (int rc = band_cnlp_attach(b, nlp, nterms, t_row, t_j, t_k, t_w)) {
      fpsq_band_nlp_destroy(nlp);
      return rc;
    }
  }
  *out = nlp;
  return FPSQ_OK;
}

}  // extern "C"
