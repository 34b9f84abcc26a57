// elem_walk.h -- the element loop and the canonical strains of the kernels that read a cell's correctors with one workgroup per macro
// cell and elements on lanes (sensitivity.hip, loads.hip, sens_strat.hip).  `Args` carries the geometry fields of ReconArgs (kernels.h).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "mesh_elem.h"
#include "struct_elem.h"

namespace hommx {

constexpr int kWalkThreads = 512;
constexpr int kWalkWaves = kWalkThreads / 64;

// f(el, vol, vertex) for the elements of this thread, ascending: the element loops of k_recon.  vertex(a, node, g): the periodic node
// and the P1 gradient of local vertex a, read (mesh plans) or computed (structured plans) when asked for
template <int DIM, bool MESH, typename Args, typename F>
__device__ __forceinline__ void for_elements(const Args& A, int tid, F&& f) {
  if constexpr (MESH) {
    for (long long el = tid; el < A.n_el; el += kWalkThreads)
      f(el, A.vol[el], [&](int a, int& node, double(&g)[DIM]) {
        node = A.el_nodes[el * (DIM + 1) + a];
#pragma unroll
        for (int k = 0; k < DIM; ++k) g[k] = A.grads[(el * (DIM + 1) + a) * DIM + k];
      });
  } else {
    // one grid cell (all its sub-simplices, element order n_sub (i + n j [+ n^2 k]) + s) per thread and step; the 3D loop stays rolled
    constexpr int NSUB = DIM == 2 ? 2 : 6;
    constexpr int UNROLL = DIM == 2 ? 2 : 1;
    const int n = A.n;
    const double hn = (double)n;
    const long long ncube = A.n_el / NSUB;
    for (long long cube = tid; cube < ncube; cube += kWalkThreads) {
      const int i = (int)(cube % n), j = (int)((cube / n) % n), k = DIM == 3 ? (int)(cube / ((long long)n * n)) : 0;
#pragma unroll UNROLL
      for (int s = 0; s < NSUB; ++s)
        f(cube * NSUB + s, A.vol_struct, [&](int a, int& node, double(&g)[DIM]) { struct_vertex<DIM>(i, j, k, s, a, n, hn, node, g); });
    }
  }
}

// s[m] = s^m_K for the t canonical loads: the arithmetic of k_recon's element<>() on chi^xi = chi_m.  3D elasticity takes one vertex at
// a time (a rolled loop): its 72 gathers in flight at once would not leave registers for the 36 strains and the running sums
// CANON false: the strains of the fields alone, without the unit load in front (the correctors of user-supplied loads: loads.hip), and
// of the first `rows` fields only (uniform over the workgroup); the other rows of s are zero and their fields are not read
template <int DIM, int KIND, bool CANON = true, typename V>
__device__ __forceinline__ void load_strains(const double* __restrict__ corr, long long ndof, V&& vertex, const double* Mc,
                                             double (&s)[kind_sizes(DIM, KIND).t][kind_sizes(DIM, KIND).t], int rows = kind_sizes(DIM, KIND).t) {
  constexpr KindSizes ks = kind_sizes(DIM, KIND);
  constexpr int T = ks.t, BS = ks.bs, VERTS = T == 6 ? 1 : DIM + 1;
#pragma unroll
  for (int m = 0; m < T; ++m)
#pragma unroll
    for (int k = 0; k < T; ++k) s[m][k] = CANON && m == k ? 1.0 : 0.0;
#pragma unroll VERTS
  for (int a = 0; a < DIM + 1; ++a) {
    int node;
    double g[DIM];
    vertex(a, node, g);
#pragma unroll
    for (int al = 0; al < BS; ++al) {
      double sa[T];
      strain<DIM, KIND>(g, Mc, al, sa);
      const double* __restrict__ at = corr + (long long)node * BS + al;
#pragma unroll
      for (int m = 0; m < T; ++m)
        if (CANON || m < rows) {
          const double c = at[m * ndof];
#pragma unroll
          for (int k = 0; k < T; ++k) s[m][k] += c * sa[k];
        }
    }
  }
}

// H[n][alpha][b] = sum_a chi_n[p_a bs + alpha] g_a[b]: the raw gradient of the first COUNT fields of `corr` on the element, M not applied
// (sens_strat.hip).  Six fields of 3D elasticity take one vertex at a time, as in load_strains
template <int DIM, int KIND, int COUNT, typename V>
__device__ __forceinline__ void load_gradients(const double* __restrict__ corr, long long ndof, V&& vertex,
                                               double (&H)[COUNT][kind_sizes(DIM, KIND).bs][DIM]) {
  constexpr int BS = kind_sizes(DIM, KIND).bs, VERTS = COUNT == 6 ? 1 : DIM + 1;
#pragma unroll
  for (int n = 0; n < COUNT; ++n)
#pragma unroll
    for (int al = 0; al < BS; ++al)
#pragma unroll
      for (int b = 0; b < DIM; ++b) H[n][al][b] = 0.0;
#pragma unroll VERTS
  for (int a = 0; a < DIM + 1; ++a) {
    int node;
    double g[DIM];
    vertex(a, node, g);
#pragma unroll
    for (int al = 0; al < BS; ++al) {
      const double* __restrict__ at = corr + (long long)node * BS + al;
#pragma unroll
      for (int n = 0; n < COUNT; ++n) {
        const double c = at[n * ndof];
#pragma unroll
        for (int b = 0; b < DIM; ++b) H[n][al][b] += c * g[b];
      }
    }
  }
}

}  // namespace hommx
