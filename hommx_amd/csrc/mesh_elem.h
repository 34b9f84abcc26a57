// mesh_elem.h -- element formulas of the mesh routes (mesh_front.hip: frontal kernel, mesh_tree.hip: assembly kernel of the tree route):
// the material matrix of an element and the strain of one of its local dofs, both in the basis of the canonical loads.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/hommx_hip.h"

namespace hommx {

// Material matrix C (t x t) of an element in the basis of the canonical loads (Poisson: A; elasticity: E^m : A : E^n).
template <int DIM, int KIND>
__device__ __forceinline__ void material(const double* __restrict__ c, double (&C)[KIND >= 2 ? DIM * (DIM + 1) / 2 : DIM][KIND >= 2 ? DIM * (DIM + 1) / 2 : DIM]) {
  constexpr int T = KIND >= 2 ? DIM * (DIM + 1) / 2 : DIM;
  if constexpr (KIND == HOMMX_KIND_POISSON_SCALAR) {
    const double a = c[0];
#pragma unroll
    for (int m = 0; m < T; ++m)
#pragma unroll
      for (int n = 0; n < T; ++n) C[m][n] = m == n ? a : 0.0;
  } else if constexpr (KIND == HOMMX_KIND_POISSON_MATRIX) {
    // (00, 11, [22,] 01 [, 02, 12])
#pragma unroll
    for (int m = 0; m < DIM; ++m) C[m][m] = c[m];
    C[0][1] = C[1][0] = c[DIM];
    if constexpr (DIM == 3) {
      C[0][2] = C[2][0] = c[4];
      C[1][2] = C[2][1] = c[5];
    }
  } else if constexpr (KIND == HOMMX_KIND_ELASTICITY_ISO) {
    const double lam = c[0], mu = c[1];
#pragma unroll
    for (int m = 0; m < T; ++m)
#pragma unroll
      for (int n = 0; n < T; ++n) C[m][n] = (m < DIM && n < DIM ? lam : 0.0) + (m == n ? (m < DIM ? 2.0 * mu : mu) : 0.0);
  } else {
    // upper triangle of the t x t matrix, row-major
    int q = 0;
#pragma unroll
    for (int m = 0; m < T; ++m)
#pragma unroll
      for (int n = m; n < T; ++n, ++q) C[m][n] = C[n][m] = c[q];
  }
}

// entry C[m][n] of material(c), n uniform and not a constant (m may be one): the same value as material() gives, read or formed where
// it is needed, so that a caller holds a few columns instead of the matrix
template <int DIM, int KIND>
__device__ __forceinline__ double material_entry(const double* __restrict__ c, int m, int n) {
  constexpr int T = KIND >= 2 ? DIM * (DIM + 1) / 2 : DIM;
  if constexpr (KIND == HOMMX_KIND_POISSON_SCALAR) {
    return m == n ? c[0] : 0.0;
  } else if constexpr (KIND == HOMMX_KIND_POISSON_MATRIX) {
    return m == n ? c[m] : c[DIM + (m + n - 1)];  // 01, 02, 12 behind the diagonal
  } else if constexpr (KIND == HOMMX_KIND_ELASTICITY_ISO) {
    const double lam = c[0], mu = c[1];
    return (m < DIM && n < DIM ? lam : 0.0) + (m == n ? (m < DIM ? 2.0 * mu : mu) : 0.0);
  } else {
    const int r = m < n ? m : n, s = m < n ? n : m;
    return c[r * T - r * (r - 1) / 2 + (s - r)];
  }
}

// g = material(unit_k) e, the column of the (linear) map c -> material(c) e at entry k of the coefficient; k is uniform over the wave and
// no register array is indexed with it.  The operation order, which SecantLaw._material_columns (hommx_amd/expr.py) follows: every
// entry of g is one entry of e, copied, or +0.0, except
//   the Lame pair: k = 0 (lambda): g[m] = (e[0] + e[1]) (+ e[2], added last) on the normal rows m < DIM, +0.0 on the shear rows;
//                  k = 1 (mu): g[m] = 2 e[m] (one product) on the normal rows, e[m] on the shear rows.
// Scalar: g = e.  Matrix (00, 11, [22,] 01 [, 02, 12]) and Voigt (upper triangle, row-major): entry k = (r, c), r <= c, gives
// g[r] = e[c] and g[c] = e[r]
template <int DIM, int KIND>
__device__ __forceinline__ void material_column(int k, const double (&e)[KIND >= 2 ? DIM * (DIM + 1) / 2 : DIM],
                                                double (&g)[KIND >= 2 ? DIM * (DIM + 1) / 2 : DIM]) {
#pragma clang fp contract(off)
  constexpr int T = KIND >= 2 ? DIM * (DIM + 1) / 2 : DIM;
  if constexpr (KIND == HOMMX_KIND_POISSON_SCALAR) {
#pragma unroll
    for (int m = 0; m < T; ++m) g[m] = e[m];
  } else if constexpr (KIND == HOMMX_KIND_ELASTICITY_ISO) {
    double tr = e[0] + e[1];
    if constexpr (DIM == 3) tr = tr + e[2];
#pragma unroll
    for (int m = 0; m < T; ++m) g[m] = k == 0 ? (m < DIM ? tr : 0.0) : (m < DIM ? 2.0 * e[m] : e[m]);
  } else {
    // (r, c) of entry k: a scan over the constant pairs in the kind's order
    int r = 0, c = 0;
    if constexpr (KIND == HOMMX_KIND_POISSON_MATRIX) {
      const int o = k - DIM;  // the off-diagonal pairs 01, 02, 12
      r = k < DIM ? k : o == 2 ? 1 : 0;
      c = k < DIM ? k : o == 0 ? 1 : 2;
    } else {
      int q = 0;
#pragma unroll
      for (int m = 0; m < T; ++m)
#pragma unroll
        for (int n = m; n < T; ++n, ++q)
          if (q == k) {
            r = m;
            c = n;
          }
    }
    double er = e[0], ec = e[0];
#pragma unroll
    for (int m = 1; m < T; ++m) {
      er = m == r ? e[m] : er;
      ec = m == c ? e[m] : ec;
    }
#pragma unroll
    for (int m = 0; m < T; ++m) g[m] = m == r ? ec : m == c ? er : 0.0;
  }
}

// strain of local dof r = a * bs + alpha in the basis of the canonical loads: Poisson M g_a; elasticity sym(e_alpha (x) M g_a) with
// the off-diagonal components doubled (E^m, m = (k, l), k != l, has 1/2 at kl and lk)
template <int DIM, int KIND>
__device__ __forceinline__ void strain(const double* __restrict__ g, const double* __restrict__ M, int alpha,
                                       double (&s)[KIND >= 2 ? DIM * (DIM + 1) / 2 : DIM]) {
  double gt[DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i) {
    if (M) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < DIM; ++k) v += M[i * DIM + k] * g[k];
      gt[i] = v;
    } else {
      gt[i] = g[i];
    }
  }
  if constexpr (KIND < 2) {
#pragma unroll
    for (int i = 0; i < DIM; ++i) s[i] = gt[i];
  } else {
#pragma unroll
    for (int m = 0; m < DIM; ++m) s[m] = alpha == m ? gt[m] : 0.0;
    constexpr int PK[3] = {0, 0, 1}, PL[3] = {1, 2, 2};  // Voigt pairs 01, 02, 12
#pragma unroll
    for (int o = 0; o < DIM * (DIM - 1) / 2; ++o) {
      const int k = PK[o], l = PL[o];
      s[DIM + o] = (alpha == k ? gt[l] : 0.0) + (alpha == l ? gt[k] : 0.0);
    }
  }
}

}  // namespace hommx
