// sens_strat.hip -- derivatives of the effective tensor with respect to the stratification M.
//
// For macro cell c with canonical correctors chi_n, H^n_K[alpha][b] = sum_a chi_n[p_a bs + alpha] g_a[b] is the raw gradient of corrector n
// on micro element K (no M), s^n_K = e_n + voigt(H^n_K M^T) its strain under the canonical load e_n (M applied, shear doubled: the s^n_K of
// sensitivity.hip) and sigma^n_K = material(coef_K) s^n_K its flux / stress.  The strain is linear in M and C0 does not depend on it, so
//   dA_dM[c][a][b][m][n] = sum_K |K| [ (sigma^m_K H^n_K)[a][b] + (sigma^n_K H^m_K)[a][b] ]    (no derivative of a corrector: the cell equation)
//   grad_M[c][a][b]      = sum_{m,n} w[c][m][n] dA_dM[c][a][b][m][n] = sum_K |K| sum_n (V^n_K H^n_K)[a][b],  V^n = sum_m (w[m][n] + w[n][m]) sigma^m
// with sigma the d x bs matrix sigma[a][alpha] (Poisson: the flux vector, bs = 1; elasticity: the symmetric tensor of the Voigt vector,
// shear not doubled).
//
// One workgroup per macro cell, elements on lanes, the correctors gathered from global memory as k_sens gathers them.  The t (t + 1) / 2
// running sums of all d d entries (a, b) fit the registers of every kind but 3D elasticity (t = 6: 9 x 21 sums), which takes one pass over
// the elements per (a, b); the gradient is one more pass with d d sums and no t x t intermediate.  The fixed-order sums of elem_walk.h
// (block_sums), m <= n computed and mirrored: a cell's outputs do not depend on its batch position, the chunking or which outputs are
// asked for.  No atomics, no inline assembly.
#include <hip/hip_runtime.h>

#include "elem_walk.h"
#include "kernels.h"

namespace hommx {

namespace {

// entries (a, b) of dA_dM per pass over the elements
constexpr int pass_group(int dim, int kind) { return kind_sizes(dim, kind).t == 6 ? 1 : dim * dim; }

// v[i] of a register array for an index that is uniform over the workgroup but not known to the compiler: selects between values, no
// loop, so that the array is split into registers before anything addresses it
template <int DIM>
__device__ __forceinline__ double pick(const double (&v)[DIM], int i) {
  const double v0 = v[0], v1 = v[1];
  if constexpr (DIM == 2) {
    return i == 1 ? v1 : v0;
  } else {
    const double v2 = v[2];
    return i == 2 ? v2 : (i == 1 ? v1 : v0);
  }
}

// position of sigma[a][alpha] in the Voigt vector (00, 11, [22,] 01 [, 02, 12])
template <int DIM>
__device__ __forceinline__ constexpr int voigt(int a, int al) {
  return a == al ? a : DIM + a + al - 1;
}

// Voigt vector sv of material(coef_K) (e + voigt(Hn M^T)): the flux / stress of the field with raw gradient Hn under the macro load e
template <int DIM, int KIND>
__device__ __forceinline__ void stress(const double (&Hn)[kind_sizes(DIM, KIND).bs][DIM], const double* Mp,
                                       const double (&C)[kind_sizes(DIM, KIND).t][kind_sizes(DIM, KIND).t],
                                       const double (&e)[kind_sizes(DIM, KIND).t], double (&sv)[kind_sizes(DIM, KIND).t]) {
  constexpr KindSizes ks = kind_sizes(DIM, KIND);
  constexpr int T = ks.t, BS = ks.bs;
  double G[BS][DIM], s[T];  // G = Hn M^T, the gradient in the stratified frame
#pragma unroll
  for (int al = 0; al < BS; ++al)
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < DIM; ++k) v += Mp[i * DIM + k] * Hn[al][k];
      G[al][i] = v;
    }
  if constexpr (KIND < 2) {
#pragma unroll
    for (int i = 0; i < DIM; ++i) s[i] = e[i] + G[0][i];
  } else {
#pragma unroll
    for (int k = 0; k < DIM; ++k)
#pragma unroll
      for (int l = k; l < DIM; ++l) s[voigt<DIM>(k, l)] = e[voigt<DIM>(k, l)] + (k == l ? G[k][k] : G[k][l] + G[l][k]);
  }
#pragma unroll
  for (int k = 0; k < T; ++k) {
    double v = 0.0;
#pragma unroll
    for (int l = 0; l < T; ++l) v += C[k][l] * s[l];
    sv[k] = v;
  }
}

// sigma^n[a][alpha] of the Voigt vector sv; a uniform over the workgroup
template <int DIM, int KIND>
__device__ __forceinline__ double stress_entry(const double (&sv)[kind_sizes(DIM, KIND).t], int a, int al) {
  if constexpr (KIND < 2) {
    return pick<DIM>(sv, a);
  } else {
    double row[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) row[k] = sv[voigt<DIM>(k, al)];
    return pick<DIM>(row, a);
  }
}

template <int DIM, int KIND, bool MESH>
__global__ __launch_bounds__(kWalkThreads) void k_sens_strat(StratSensArgs A) {
  constexpr KindSizes ks = kind_sizes(DIM, KIND);
  constexpr int T = ks.t, BS = ks.bs, NCOMP = ks.n_comp;
  constexpr int NSUM = T * (T + 1) / 2;  // dA_dM[a][b][m][n], m <= n, at n (n + 1) / 2 + m
  constexpr int GROUP = pass_group(DIM, KIND), NACC = GROUP * NSUM > DIM * DIM ? GROUP * NSUM : DIM * DIM;
  __shared__ double red[kWalkWaves * NACC];  // the rows of block_sums, of either pass
  const int tid = threadIdx.x;
  const long long cell = blockIdx.x;
  const double* corr = A.corr + cell * T * A.ndof;
  const double* coef = A.coef + cell * A.n_el * NCOMP;

  double Mp[DIM * DIM];
  cell_M<DIM>(A.M, cell, Mp);

  if (A.dA_dM) {
    for (int ab0 = 0; ab0 < DIM * DIM; ab0 += GROUP) {
      double acc[GROUP * NSUM];
#pragma unroll
      for (int q = 0; q < GROUP * NSUM; ++q) acc[q] = 0.0;
      for_elements<DIM, MESH>(A, tid, [&](long long el, double vol, auto vertex) {
        double H[T][BS][DIM], C[T][T];
        load_gradients<DIM, KIND, T>(corr, A.ndof, vertex, H);
        material<DIM, KIND>(coef + el * NCOMP, C);
        // sigma^n[a][.] and H^n[.][b] of the entries (a, b) of this pass, one corrector at a time: H^n is dead once they are taken
        double sa[GROUP][T][BS], hb[GROUP][T][BS];
#pragma unroll
        for (int n = 0; n < T; ++n) {
          double e[T], sv[T];
#pragma unroll
          for (int k = 0; k < T; ++k) e[k] = k == n ? 1.0 : 0.0;
          stress<DIM, KIND>(H[n], Mp, C, e, sv);
#pragma unroll
          for (int g = 0; g < GROUP; ++g) {
            const int a = (ab0 + g) / DIM, b = (ab0 + g) % DIM;  // constants where one pass takes every entry
#pragma unroll
            for (int al = 0; al < BS; ++al) {
              sa[g][n][al] = stress_entry<DIM, KIND>(sv, a, al);
              hb[g][n][al] = pick<DIM>(H[n][al], b);
            }
          }
        }
#pragma unroll
        for (int g = 0; g < GROUP; ++g)
#pragma unroll
          for (int n = 0; n < T; ++n)
#pragma unroll
            for (int m = 0; m <= n; ++m) {
              double v = 0.0;
#pragma unroll
              for (int al = 0; al < BS; ++al) v += sa[g][m][al] * hb[g][n][al] + sa[g][n][al] * hb[g][m][al];
              acc[g * NSUM + n * (n + 1) / 2 + m] += vol * v;
            }
      });
      double* out = A.dA_dM + (cell * DIM * DIM + ab0) * T * T;
      block_sums<GROUP * NSUM>(acc, reinterpret_cast<double(*)[GROUP * NSUM]>(red), tid, [&](int q, double total) {
        const int g = q / NSUM, n = tri_row(q % NSUM), m = q % NSUM - n * (n + 1) / 2;
        out[(g * T + m) * T + n] = out[(g * T + n) * T + m] = total;
      });
      __syncthreads();  // the next pass writes `red` again
    }
  }

  if (A.grad_M) {
    double w[NSUM];  // w[m][n] + w[n][m], m <= n, at n (n + 1) / 2 + m: uniform over the cell
#pragma unroll
    for (int n = 0; n < T; ++n)
#pragma unroll
      for (int m = 0; m <= n; ++m) w[n * (n + 1) / 2 + m] = A.weights[cell * T * T + m * T + n] + A.weights[cell * T * T + n * T + m];
    auto ws = [&](int m, int n) { return m <= n ? w[n * (n + 1) / 2 + m] : w[m * (m + 1) / 2 + n]; };
    double acc[DIM * DIM];
#pragma unroll
    for (int q = 0; q < DIM * DIM; ++q) acc[q] = 0.0;
    for_elements<DIM, MESH>(A, tid, [&](long long el, double vol, auto vertex) {
      double H[T][BS][DIM], C[T][T];
      load_gradients<DIM, KIND, T>(corr, A.ndof, vertex, H);
      material<DIM, KIND>(coef + el * NCOMP, C);
#pragma unroll
      for (int n = 0; n < T; ++n) {
        // V^n = sum_m ws(m, n) sigma^m, by linearity the stress of the field sum_m ws(m, n) chi_m under the load ws(., n)
        double U[BS][DIM], e[T], V[T];
#pragma unroll
        for (int al = 0; al < BS; ++al)
#pragma unroll
          for (int b = 0; b < DIM; ++b) {
            double v = 0.0;
#pragma unroll
            for (int m = 0; m < T; ++m) v += ws(m, n) * H[m][al][b];
            U[al][b] = v;
          }
#pragma unroll
        for (int m = 0; m < T; ++m) e[m] = ws(m, n);
        stress<DIM, KIND>(U, Mp, C, e, V);
#pragma unroll
        for (int k = 0; k < T; ++k) V[k] *= vol;
#pragma unroll
        for (int a = 0; a < DIM; ++a)
#pragma unroll
          for (int b = 0; b < DIM; ++b)
#pragma unroll
            for (int al = 0; al < BS; ++al) acc[a * DIM + b] += stress_entry<DIM, KIND>(V, a, al) * H[n][al][b];
      }
    });
    double* out = A.grad_M + cell * DIM * DIM;
    block_sums<DIM * DIM>(acc, reinterpret_cast<double(*)[DIM * DIM]>(red), tid, [&](int q, double total) { out[q] = total; });
  }
}

}  // namespace

hipError_t launch_sens_strat(const StratSensArgs& a, long long nc, hipStream_t st) {
  return launch_walk(a, nc, st, walk_kernel(a, [](auto D, auto K, auto MESH) { return &k_sens_strat<D(), K(), MESH()>; }));
}

}  // namespace hommx
