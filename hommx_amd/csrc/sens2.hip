// sens2.hip -- second derivatives of the effective tensor along coefficient directions.
//
// With s^m_K = e_m + eps(chi^m)_K the canonical strains (sensitivity.hip) and the element operator linear in the coefficient, the
// derivative of the canonical corrector m along a perturbation dir_b of the element stream is the corrector of a polarisation load:
//   load        P^{b,m}_K = material(dir_b[K]) s^m_K                         k_sens2_loads: into plan scratch, as a per-cell load block
//   corrector   K chi^m_b = -f(P^{b,m})                                      the load solve of loads.hip / fused2d_rhs.hip, between the two
//   g_ab[m][n]  = sum_K |K| eps(chi^m_b)_K . material(dir_a[K]) s^n_K        k_sens2: for every a <= b
//   d2A[a][b]   = g_ab + g_ab^T = d2A[b][a]                                  formed once and mirrored: symmetric bitwise in (m, n) and (a, b)
// There is no second derivative of the operator.  P is in flux / stress components (shear not doubled), the strains have the shear
// doubled: the conventions of loads.hip.
//
// Both kernels: one workgroup per macro cell, elements on lanes, correctors gathered from global memory (elem_walk.h).  k_sens2_loads has
// no reduction; every element writes its t loads.  k_sens2 takes one pass over the elements per a <= b: the t x t canonical strains stay
// in registers, the strain of one load corrector at a time is gathered in a rolled loop and its row of the t x t sums picked by selects
// (k_polar's device), so that 3D elasticity (t = 6) fits the registers.  Sums: the fixed-order sums of elem_walk.h (block_sums) -- a
// cell's outputs do not depend on its batch position or the chunking.  No atomics, no inline assembly.
#include <hip/hip_runtime.h>

#include "elem_walk.h"
#include "kernels.h"

namespace hommx {

namespace {

// P[cell][m][K] = material(dir_b[K]) s^m_K for the t canonical loads: a per-cell load block of hommx_loads_source.  Lane K writes the t
// components of its element next to those of lane K + 1
template <int DIM, int KIND, bool MESH>
__global__ __launch_bounds__(kWalkThreads) void k_sens2_loads(Sens2Args A) {
  constexpr KindSizes ks = kind_sizes(DIM, KIND);
  constexpr int T = ks.t, NCOMP = ks.n_comp;
  const int tid = threadIdx.x;
  const long long cell = blockIdx.x;
  const double* corr = A.corr + cell * T * A.ndof;
  const double* dir = A.dirs + ((A.per_cell ? cell * A.n_dirs : 0) + A.b) * A.n_el * NCOMP;
  double* P = A.P + cell * T * A.n_el * T;
  double Mp[DIM * DIM];
  cell_M<DIM>(A.M, cell, Mp);
  for_elements<DIM, MESH>(A, tid, [&](long long el, double, auto vertex) {
    double s[T][T], C[T][T];
    load_strains<DIM, KIND>(corr, A.ndof, vertex, Mp, s);
    material<DIM, KIND>(dir + el * NCOMP, C);
#pragma unroll
    for (int m = 0; m < T; ++m) {
      double* __restrict__ pk = P + ((long long)m * A.n_el + el) * T;
#pragma unroll
      for (int k = 0; k < T; ++k) {
        double v = 0.0;
#pragma unroll
        for (int l = 0; l < T; ++l) v += C[k][l] * s[m][l];
        pk[k] = v;
      }
    }
  });
}

// d2A[cell][a][b] and its mirror d2A[cell][b][a] for every a <= b = A.b, from the canonical correctors and the load correctors of dir_b
template <int DIM, int KIND, bool MESH>
__global__ __launch_bounds__(kWalkThreads) void k_sens2(Sens2Args A) {
  constexpr KindSizes ks = kind_sizes(DIM, KIND);
  constexpr int T = ks.t, NCOMP = ks.n_comp, NSUM = T * T;
  __shared__ double red[kWalkWaves][NSUM];
  __shared__ double g[T * T];  // g_ab[m][n], the totals
  const int tid = threadIdx.x;
  const long long cell = blockIdx.x;
  const double* corr = A.corr + cell * T * A.ndof;
  const double* corr_b = A.corr_b + cell * T * A.ndof;
  const int b = A.b, nd = A.n_dirs;
  double Mp[DIM * DIM];
  cell_M<DIM>(A.M, cell, Mp);

  for (int a = 0; a <= b; ++a) {
    const double* dir = A.dirs + ((A.per_cell ? cell * nd : 0) + a) * A.n_el * NCOMP;
    double acc[NSUM];  // g_ab[m][n], this thread's elements
#pragma unroll
    for (int q = 0; q < NSUM; ++q) acc[q] = 0.0;
    for_elements<DIM, MESH>(A, tid, [&](long long el, double vol, auto vertex) {
      double s[T][T], C[T][T];
      load_strains<DIM, KIND>(corr, A.ndof, vertex, Mp, s);
      material<DIM, KIND>(dir + el * NCOMP, C);
      // one load corrector at a time (a rolled loop: the 36 strains of six of them beside the 36 canonical strains, the operator and
      // the 36 sums of 3D elasticity do not fit the registers); row m of the sums is picked by selects over the unrolled rows
#pragma unroll 1
      for (int m = 0; m < T; ++m) {
        double eb[T][T], ce[T];  // row 0: eps(chi^m_b)_K; material(dir_a[K]) eps(chi^m_b)_K (the operator is symmetric)
        load_strains<DIM, KIND, false>(corr_b + (long long)m * A.ndof, A.ndof, vertex, Mp, eb, 1);
#pragma unroll
        for (int k = 0; k < T; ++k) {
          double v = 0.0;
#pragma unroll
          for (int l = 0; l < T; ++l) v += C[k][l] * eb[0][l];
          ce[k] = v;
        }
#pragma unroll
        for (int n = 0; n < T; ++n) {
          double v = 0.0;
#pragma unroll
          for (int k = 0; k < T; ++k) v += ce[k] * s[n][k];
          v *= vol;
#pragma unroll
          for (int q = 0; q < T; ++q) acc[q * T + n] = q == m ? acc[q * T + n] + v : acc[q * T + n];
        }
      }
    });
    // thread q takes total q: one thread holding all t^2 totals beside its sums spills at t = 6
    const double total = block_sums<NSUM>(acc, red, tid, NSUM);
    if (tid < NSUM) g[tid] = total;
    __syncthreads();
    // g + g^T once per pair m <= n, stored at its four places
    if (tid < T * T) {
      const int m = tid / T, n = tid % T;
      if (m <= n) {
        const double v = g[m * T + n] + g[n * T + m];
        double* ab = A.d2A + ((cell * nd + a) * nd + b) * T * T;
        double* ba = A.d2A + ((cell * nd + b) * nd + a) * T * T;
        ab[m * T + n] = ab[n * T + m] = v;
        ba[m * T + n] = ba[n * T + m] = v;
      }
    }
    __syncthreads();  // the next direction writes red and g again
  }
}

// d2A[cell][a][b][q] = add(d2A[cell][a][b][q], dAk[cell][pair(a, b)][q]), q < t t, for every (a, b): the curvature term of
// HOMMX_DIRS_PARAMETERS_CURVATURE.  One thread per entry of d2A; (a, b) and (b, a) take the same addend and dAk is symmetric in (m, n)
// bitwise (k_sens mirrors it), so the bitwise symmetries of d2A survive
__global__ __launch_bounds__(256) void k_sens2_add_curvature(double* __restrict__ d2A, const double* __restrict__ dAk, int nd, int tt,
                                                             long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int q = (int)(idx % tt);
  const long long r = idx / tt;
  const int b = (int)(r % nd), a = (int)((r / nd) % nd);
  const long long cell = r / ((long long)nd * nd);
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  const int pair = lo * nd - lo * (lo - 1) / 2 + (hi - lo), n_pairs = nd * (nd + 1) / 2;  // row-major over lo <= hi
  d2A[idx] = add_rn(d2A[idx], dAk[(cell * n_pairs + pair) * tt + q]);
}

}  // namespace

hipError_t launch_sens2_add_curvature(double* d2A, const double* dAk, int n_dirs, int t, long long nc, hipStream_t st) {
  const long long total = nc * n_dirs * n_dirs * t * t;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_sens2_add_curvature, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d2A, dAk, n_dirs, t * t, total);
  return hipGetLastError();
}

hipError_t launch_sens2_loads(const Sens2Args& a, long long nc, hipStream_t st) {
  return launch_walk(a, nc, st, walk_kernel(a, [](auto D, auto K, auto MESH) { return &k_sens2_loads<D(), K(), MESH()>; }));
}

hipError_t launch_sens2(const Sens2Args& a, long long nc, hipStream_t st) {
  return launch_walk(a, nc, st, walk_kernel(a, [](auto D, auto K, auto MESH) { return &k_sens2<D(), K(), MESH()>; }));
}

}  // namespace hommx
