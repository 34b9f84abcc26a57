// elem_walk.h -- what the kernels that read a cell's correctors with one workgroup per macro cell and elements on lanes share
// (reconstruct.hip, sensitivity.hip, sens2.hip, sens_strat.hip, loads.hip): the element loop, M of the cell, the canonical strains, the
// fixed-order reductions and the launcher.  Their argument structs derive from ElemWalk (kernels.h).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "mesh_elem.h"
#include "struct_elem.h"

namespace hommx {

constexpr int kWalkThreads = 512;
constexpr int kWalkWaves = kWalkThreads / 64;

// f(el, vol, vertex) for the elements of this thread, ascending.  vertex(a, node, g): the periodic node and the P1 gradient of local
// vertex a, read (mesh plans) or computed (structured plans) when asked for
template <int DIM, bool MESH, typename F>
__device__ __forceinline__ void for_elements(const ElemWalk& A, int tid, F&& f) {
  if constexpr (MESH) {
    for (long long el = tid; el < A.n_el; el += kWalkThreads)
      f(el, A.vol[el], [&](int a, int& node, double(&g)[DIM]) {
        node = A.el_nodes[el * (DIM + 1) + a];
#pragma unroll
        for (int k = 0; k < DIM; ++k) g[k] = A.grads[(el * (DIM + 1) + a) * DIM + k];
      });
  } else {
    // one grid cell (all its sub-simplices, element order n_sub (i + n j [+ n^2 k]) + s) per thread and step; six tetrahedra unrolled
    // hold too many registers: the 3D loop stays rolled, its tables read from constant memory
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

// M of the cell, or the identity (exact: the same gradients as without M); one private array that never escapes, so it stays in registers
template <int DIM>
__device__ __forceinline__ void cell_M(const double* M, long long cell, double (&Mp)[DIM * DIM]) {
#pragma unroll
  for (int k = 0; k < DIM * DIM; ++k) Mp[k] = M ? M[cell * DIM * DIM + k] : (k % (DIM + 1) == 0 ? 1.0 : 0.0);
}

// row n of position q = n (n + 1) / 2 + m, m <= n, of the packed triangle the symmetric t x t sums are kept in
__device__ constexpr int tri_row(int q) {
  int n = 0;
  while ((n + 1) * (n + 2) / 2 <= q) ++n;
  return n;
}

// The fixed order of every sum over a cell: element-strided partial sums per thread (for_elements), a butterfly in each wave, the wave
// totals in ascending order.  A cell's outputs therefore do not depend on its batch position, the chunking or which outputs are asked
// for, and the tests hold that bit for bit.  wave_sums is what both forms of block_sums begin with: the butterfly of v[q], the totals
// of wave w into red[w], the barrier
template <int N>
__device__ __forceinline__ void wave_sums(double (&v)[N], double (*red)[N], int tid) {
#pragma unroll
  for (int q = 0; q < N; ++q)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v[q] += __shfl_xor(v[q], o, 64);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int q = 0; q < N; ++q) red[tid >> 6][q] = v[q];
  }
  __syncthreads();
}
// thread 0 hands total q to out(q, total), q ascending and a constant once unrolled: a total that is stored at once holds no register
// while the next one is added up
template <int N, typename Out>
__device__ __forceinline__ void block_sums(double (&v)[N], double (*red)[N], int tid, Out&& out) {
  wave_sums<N>(v, red, tid);
  if (tid == 0) {
#pragma unroll
    for (int q = 0; q < N; ++q) {
      double t = red[0][q];
      for (int w = 1; w < kWalkWaves; ++w) t += red[w][q];
      out(q, t);
    }
  }
}
// thread q < count returns total q (one thread holding all t^2 totals beside its sums spills at t = 6)
template <int N>
__device__ __forceinline__ double block_sums(double (&v)[N], double (*red)[N], int tid, int count) {
  wave_sums<N>(v, red, tid);
  double t = 0.0;
  if (tid < count) {
    t = red[0][tid];
    for (int w = 1; w < kWalkWaves; ++w) t += red[w][tid];
  }
  return t;
}

// The largest norm of a cell and the element reaching it, in the same order.  The rule: the larger norm wins, ties go to the smaller
// non-negative element (-1: a thread that saw none).  Thread 0 returns with both in (mx, arg); the barrier in it covers red alone
__device__ __forceinline__ void block_argmax(double& mx, double& arg, double (*red)[2], int tid) {
  auto take = [&](double omx, double oarg) {
    if (omx > mx || (omx == mx && oarg < arg && oarg >= 0)) {
      mx = omx;
      arg = oarg;
    }
  };
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) take(__shfl_xor(mx, o, 64), __shfl_xor(arg, o, 64));
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = mx;
    red[tid >> 6][1] = arg;
  }
  __syncthreads();
  if (tid == 0)
    for (int w = 1; w < kWalkWaves; ++w) take(red[w][0], red[w][1]);
}

// The N largest-value reductions of a cell in the same order; EVERY thread returns with the totals in v (each reads the wave rows
// itself), so the workgroup can branch on them without a second barrier.  A NaN never wins
template <int N>
__device__ __forceinline__ void block_maxima(double (&v)[N], double (*red)[N], int tid) {
  auto take = [](double& m, double o) {
    if (o > m) m = o;
  };
#pragma unroll
  for (int q = 0; q < N; ++q)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) take(v[q], __shfl_xor(v[q], o, 64));
  if ((tid & 63) == 0) {
#pragma unroll
    for (int q = 0; q < N; ++q) red[tid >> 6][q] = v[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < N; ++q) {
    v[q] = red[0][q];
    for (int w = 1; w < kWalkWaves; ++w) take(v[q], red[w][q]);
  }
}

// The kernel that pick(DIM, KIND, MESH) names for the plan of `a` (integral constants; the eight pairs of dispatch_dim_kind times the
// two geometries), and its launch on nc workgroups of kWalkThreads with `lds` bytes of dynamic LDS
template <typename Args, typename Pick>
auto walk_kernel(const Args& a, Pick pick) {
  using Kernel = void (*)(Args);
  return dispatch_dim_kind(a.dim, a.kind, [&](auto D, auto K) -> Kernel {
    return a.mesh ? pick(D, K, std::true_type{}) : pick(D, K, std::false_type{});
  });
}
template <typename Args>
hipError_t launch_walk(const Args& a, long long nc, hipStream_t st, void (*kernel)(Args), size_t lds = 0) {
  if (nc <= 0) return hipSuccess;
  hipLaunchKernelGGL(kernel, dim3((unsigned)nc), dim3(kWalkThreads), lds, st, a);
  return hipGetLastError();
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
