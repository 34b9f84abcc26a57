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
