// sensitivity.hip -- derivatives of the effective tensor with respect to the micro coefficient.
//
// For macro cell c with canonical correctors chi_m, the strain of micro element K under the canonical load e_m is
//   s^m_K = e_m + sum_a sum_alpha chi_m[p_a bs + alpha] strain(g_a, M, alpha)        (k_recon's s_K for xi = e_m)
// and, the element operator being linear in the coefficient, for a perturbation dir of the element stream
//   dA[c][d][m][n] = sum_K |K| s^m_K . material(dir_d[K]) s^n_K                      (no derivative of a corrector: the cell equation)
//   grad[c][K][q]  = |K| sum_{m,n} w[c][m][n] s^m_K . material(e_q) s^n_K            (so that sum grad . dir = w : dA[dir])
// The element formulas are those of the mesh routes (mesh_elem.h), the structured geometry that of the reconstruction (struct_elem.h).
//
// One workgroup per macro cell, elements on lanes.  The t correctors of a cell are gathered from global memory, every size the same
// way: a node is shared by six (2D) to twenty-four (3D) elements of neighbouring lanes and steps, so the gathers are served by the
// caches, and a 16^3 elasticity cell (590 KB of correctors) would not fit LDS anyway.  One pass over the elements per direction -- the
// t (t + 1) / 2 running sums of eight directions do not fit the registers beside the t x t strains -- and one more for the gradient,
// which has no reduction.  dA: the fixed-order sums of elem_walk.h (block_sums), the upper triangle computed and mirrored: a cell's
// outputs do not depend on its batch position, the chunking or which outputs are asked for.  No atomics, no inline assembly.
#include <hip/hip_runtime.h>

#include "elem_walk.h"
#include "kernels.h"

namespace hommx {

namespace {

template <int DIM, int KIND, bool MESH>
__global__ __launch_bounds__(kWalkThreads) void k_sens(SensArgs A) {
  constexpr KindSizes ks = kind_sizes(DIM, KIND);
  constexpr int T = ks.t, NCOMP = ks.n_comp;
  constexpr int NSUM = T * (T + 1) / 2;  // dA[m][n], m <= n, at n (n + 1) / 2 + m
  __shared__ double red[kWalkWaves][NSUM];
  const int tid = threadIdx.x;
  const long long cell = blockIdx.x;
  const double* corr = A.corr + cell * T * A.ndof;

  double Mp[DIM * DIM];
  cell_M<DIM>(A.M, cell, Mp);

  for (int d = 0; d < A.n_dirs; ++d) {
    const double* dir = A.dirs + ((A.per_cell ? cell * A.n_dirs : 0) + d) * A.n_el * NCOMP;
    double acc[NSUM];
#pragma unroll
    for (int q = 0; q < NSUM; ++q) acc[q] = 0.0;
    for_elements<DIM, MESH>(A, tid, [&](long long el, double vol, auto vertex) {
      double s[T][T], C[T][T];
      load_strains<DIM, KIND>(corr, A.ndof, vertex, Mp, s);
      material<DIM, KIND>(dir + el * NCOMP, C);
#pragma unroll
      for (int n = 0; n < T; ++n) {
        double cs[T];  // material(dir_K) s^n
#pragma unroll
        for (int k = 0; k < T; ++k) {
          double v = 0.0;
#pragma unroll
          for (int l = 0; l < T; ++l) v += C[k][l] * s[n][l];
          cs[k] = v;
        }
#pragma unroll
        for (int m = 0; m <= n; ++m) {
          double v = 0.0;
#pragma unroll
          for (int k = 0; k < T; ++k) v += s[m][k] * cs[k];
          acc[n * (n + 1) / 2 + m] += vol * v;
        }
      }
    });

    double* out = A.dA + (cell * A.n_dirs + d) * T * T;
    block_sums<NSUM>(acc, red, tid, [&](int q, double total) {
      const int n = tri_row(q), m = q - n * (n + 1) / 2;
      out[m * T + n] = out[n * T + m] = total;
    });
    __syncthreads();  // the next pass writes `red` again
  }

  if (A.grad) {
    double w[T][T];  // uniform over the cell
#pragma unroll
    for (int m = 0; m < T; ++m)
#pragma unroll
      for (int n = 0; n < T; ++n) w[m][n] = A.weights[cell * T * T + m * T + n];
    double* grad = A.grad + cell * A.n_el * NCOMP;
    for_elements<DIM, MESH>(A, tid, [&](long long el, double vol, auto vertex) {
      double s[T][T];
      load_strains<DIM, KIND>(corr, A.ndof, vertex, Mp, s);
      // P[k][l] + P[l][k] (k < l) and P[k][k] of P = sum_{m,n} w[m][n] s^m (x) s^n: all a symmetric material(e_q) reads of it
      double P[NSUM];
#pragma unroll
      for (int q = 0; q < NSUM; ++q) P[q] = 0.0;
#pragma unroll
      for (int m = 0; m < T; ++m) {
        double u[T];  // sum_n w[m][n] s^n
#pragma unroll
        for (int l = 0; l < T; ++l) {
          double v = 0.0;
#pragma unroll
          for (int n = 0; n < T; ++n) v += w[m][n] * s[n][l];
          u[l] = v;
        }
#pragma unroll
        for (int l = 0; l < T; ++l)
#pragma unroll
          for (int k = 0; k <= l; ++k) P[l * (l + 1) / 2 + k] += k == l ? s[m][k] * u[k] : s[m][k] * u[l] + s[m][l] * u[k];
      }
#pragma unroll
      for (int q = 0; q < NCOMP; ++q) {
        double eq[NCOMP], C[T][T];
#pragma unroll
        for (int r = 0; r < NCOMP; ++r) eq[r] = r == q ? 1.0 : 0.0;
        material<DIM, KIND>(eq, C);  // constants once unrolled: only its non-zero entries cost anything
        double v = 0.0;
#pragma unroll
        for (int l = 0; l < T; ++l)
#pragma unroll
          for (int k = 0; k <= l; ++k)
            if (C[k][l] != 0.0) v += C[k][l] * P[l * (l + 1) / 2 + k];
        grad[el * NCOMP + q] = vol * v;
      }
    });
  }
}

}  // namespace

hipError_t launch_sensitivity(const SensArgs& a, long long nc, hipStream_t st) {
  return launch_walk(a, nc, st, walk_kernel(a, [](auto D, auto K, auto MESH) { return &k_sens<D(), K(), MESH()>; }));
}

}  // namespace hommx
