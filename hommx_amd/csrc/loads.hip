// loads.hip -- user-supplied polarisation loads of the periodic cell problem.
//
// Per macro cell the caller gives n_loads <= t element-wise constant fields P^l_K in R^t (flux / stress components in the order of the
// reconstruction's flux, shear not doubled).  With strain(g, M, alpha) of mesh_elem.h (shear doubled, so strain . stress is the tensor
// contraction) and s^m_K = e_m + eps(chi^m)_K the strain of element K under the canonical load m:
//   load        f^l[i bs + alpha] = sum_{K ni i} |K| P^l_K . strain(g_{a(i,K)}, M, alpha)        Brhs = -f^l: what K1 writes for P = C e_m
//   corrector   K chi_l = -f^l
//   Levin       P_eff[l][m] = sum_K |K| s^m_K . P^l_K                                            k_polar: canonical correctors alone
//   total flux  q^l_K = P^l_K + material(coef_K) eps(chi_l)_K                                    k_load_stats
//   energy      energy[l][l'] = sum_K |K| eps(chi_l)_K . material(coef_K) eps(chi_l')_K
//
// k_polar and k_load_stats: one workgroup per macro cell, elements on lanes, the correctors gathered from global memory as k_sens
// gathers them and the fixed-order reductions of elem_walk.h (block_sums, block_argmax), so a cell's outputs do not depend on its batch
// position, the chunking or which outputs are asked for.  k_assemble_loads: one thread per node gathers the load entries of its
// incident elements and writes each entry of Brhs once.  k_eigenstress: an eigenstrain E^l_K (the components and convention of the
// reconstruction's strain: shear doubled) becomes the load P^l_K = -material(coef_K) E^l_K before any of them runs, one thread per
// (cell, load, element), every entry written once.  No atomics, no inline assembly.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "blocked_internal.h"
#include "elem_walk.h"
#include "kernels.h"
#include "mesh_elem.h"

namespace hommx {

namespace {

// P[cell][l][K][:] = -(material(coef[cell][K]) E^l_K), E[cell][l][K][:] (per_cell) or E[l][K][:].  Thread i is entry (cell, l, K) with K
// fastest, so a wave reads and writes consecutive elements.  E_K is in registers before P_K is written: P may be E (per_cell only).
// Every index is a constant of an unrolled loop (the 6 x 6 matrix of 3D elasticity stays in registers)
template <int DIM, int KIND>
__global__ __launch_bounds__(256) void k_eigenstress(const double* __restrict__ coef, const double* E, bool per_cell, double* P, int n_loads,
                                                     long long n_el, long long total) {
  constexpr KindSizes ks = kind_sizes(DIM, KIND);
  constexpr int T = ks.t, NCOMP = ks.n_comp;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long long el = i % n_el, cl = i / n_el, cell = cl / n_loads, l = cl % n_loads;
  double C[T][T], e[T];
  material<DIM, KIND>(coef + (cell * n_el + el) * NCOMP, C);
  const double* ek = E + (((per_cell ? cell * n_loads : 0) + l) * n_el + el) * T;
#pragma unroll
  for (int k = 0; k < T; ++k) e[k] = ek[k];
  double* pk = P + i * T;
#pragma unroll
  for (int m = 0; m < T; ++m) {
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < T; ++k) v += C[m][k] * e[k];
    pk[m] = -v;
  }
}

// P_eff[cell][l][m] = sum_K |K| s^m_K . P^l_K: the t canonical strains of an element once, contracted with every load; P is read once
template <int DIM, int KIND, bool MESH>
__global__ __launch_bounds__(kWalkThreads) void k_polar(LoadArgs A) {
  constexpr int T = kind_sizes(DIM, KIND).t;
  __shared__ double red[kWalkWaves][T * T];
  const int tid = threadIdx.x;
  const long long cell = blockIdx.x;
  const double* corr = A.corr + cell * T * A.ndof;
  const double* P = A.P + (A.per_cell ? cell * A.n_loads : 0) * A.n_el * T;
  const int nl = A.n_loads;
  double Mp[DIM * DIM];
  cell_M<DIM>(A.M, cell, Mp);

  double acc[T * T];  // [l][m]; rows l >= n_loads stay zero
#pragma unroll
  for (int q = 0; q < T * T; ++q) acc[q] = 0.0;
  for_elements<DIM, MESH>(A, tid, [&](long long el, double vol, auto vertex) {
    double s[T][T];
    load_strains<DIM, KIND>(corr, A.ndof, vertex, Mp, s);
    // one load at a time (a rolled loop: the 36 entries of six loads in flight beside the 36 strains and the 36 sums of 3D elasticity
    // spill); row l of the sums is picked by selects over the unrolled rows, so the sums stay in registers
#pragma unroll 1
    for (int l = 0; l < nl; ++l) {
      const double* __restrict__ pk = P + ((long long)l * A.n_el + el) * T;
      double p[T];
#pragma unroll
      for (int k = 0; k < T; ++k) p[k] = pk[k];
#pragma unroll
      for (int m = 0; m < T; ++m) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < T; ++k) v += s[m][k] * p[k];
        v *= vol;
#pragma unroll
        for (int r = 0; r < T; ++r) acc[r * T + m] = r == l ? acc[r * T + m] + v : acc[r * T + m];
      }
    }
  });
  // thread q takes total q: one thread holding all t^2 totals beside its sums spills at t = 6
  const double total = block_sums<T * T>(acc, red, tid, nl * T);
  if (tid < nl * T) A.P_eff[cell * nl * T + tid] = total;
}

// The response of a cell to its loads, from their correctors chi_l (rows l < n_loads of corr).  One pass over the elements per load,
// which gathers chi_0 .. chi_l (n_loads (n_loads + 1) / 2 corrector reads per cell in all; the zero rows behind n_loads are never read) --
// the t x t strains, the material matrix and the sums of all loads at once do not fit the registers --: the mean total flux, the largest
// |q_K| (Frobenius norm for elasticity) with the smallest element reaching it, row l of the energy matrix up to the diagonal (mirrored,
// so the matrix is symmetric bitwise) and, on request, the fields of load l
template <int DIM, int KIND, bool MESH, bool FIELDS>
__global__ __launch_bounds__(kWalkThreads) void k_load_stats(LoadArgs A) {
  constexpr KindSizes ks = kind_sizes(DIM, KIND);
  constexpr int T = ks.t, NCOMP = ks.n_comp;
  constexpr int NSUM = 2 * T;  // mean flux (t) | energy[l][0 .. l] (at most t)
  __shared__ double red[kWalkWaves][NSUM], red_max[kWalkWaves][2];
  const int tid = threadIdx.x;
  const long long cell = blockIdx.x;
  const double* corr = A.corr + cell * T * A.ndof;
  const double* cc = A.coef + cell * A.n_el * NCOMP;
  const int nl = A.n_loads;
  const double* P = A.P + (A.per_cell ? cell * nl : 0) * A.n_el * T;
  double Mp[DIM * DIM];
  cell_M<DIM>(A.M, cell, Mp);

  for (int l = 0; l < nl; ++l) {
    const double* Pl = P + (long long)l * A.n_el * T;
    double* srow0 = FIELDS ? A.strain + ((cell * nl + l) * A.n_el) * T : nullptr;
    double* qrow0 = FIELDS ? A.flux + ((cell * nl + l) * A.n_el) * T : nullptr;
    double acc[NSUM];
#pragma unroll
    for (int q = 0; q < NSUM; ++q) acc[q] = 0.0;
    double mx = -1.0;
    long long arg = -1;
    for_elements<DIM, MESH>(A, tid, [&](long long el, double vol, auto vertex) {
      // separately rounded operations from here to the end of the element: which products the compiler would fuse into an fma depends on
      // the instantiation (with FIELDS the flux has a second use), and the statistics must not depend on whether fields are written.
      // The pragma covers this body alone: load_strains, strain and material are inlined with the default contraction, which both
      // instantiations see alike (every product in them has one use in either); tests/test_gpu_loads.py holds the two to the same bits
#pragma clang fp contract(off)
      double e[T][T], C[T][T];
      load_strains<DIM, KIND, false>(corr, A.ndof, vertex, Mp, e, l + 1);  // pass l needs the strains of chi_0 .. chi_l: energy[l][m <= l]
      material<DIM, KIND>(cc + el * NCOMP, C);
      double ce[T], el_strain[T];  // material(coef_K) eps(chi_l)_K; eps(chi_l)_K (l is uniform: a select over the unrolled rows)
#pragma unroll
      for (int k = 0; k < T; ++k) {
        double v = 0.0;
#pragma unroll
        for (int m = 0; m < T; ++m) v = m == l ? e[m][k] : v;
        el_strain[k] = v;
      }
#pragma unroll
      for (int k = 0; k < T; ++k) {
        double v = 0.0;
#pragma unroll
        for (int n = 0; n < T; ++n) v += C[k][n] * el_strain[n];
        ce[k] = v;
      }
      double nq = 0.0;
#pragma unroll
      for (int k = 0; k < T; ++k) {
        const double q = Pl[el * T + k] + ce[k];
        if constexpr (FIELDS) {
          srow0[el * T + k] = el_strain[k];
          qrow0[el * T + k] = q;
        }
        acc[k] += vol * q;
        nq += (KIND >= 2 && k >= DIM ? 2.0 : 1.0) * (q * q);  // Frobenius norm of sigma: shear entries twice
      }
#pragma unroll
      for (int m = 0; m < T; ++m)
        if (m <= l) {
          double v = 0.0;
#pragma unroll
          for (int k = 0; k < T; ++k) v += e[m][k] * ce[k];
          acc[T + m] += vol * v;
        }
      const double nrm = sqrt(nq);
      if (nrm > mx) {
        mx = nrm;
        arg = el;
      }
    });

    double barg = (double)arg;
    block_argmax(mx, barg, red_max, tid);
    double* st = A.stats ? A.stats + (cell * nl + l) * (T + 2) : nullptr;
    double* en = A.energy ? A.energy + cell * nl * nl : nullptr;
    block_sums<NSUM>(acc, red, tid, [&](int q, double total) {
      const int m = q - T;
      if (q < T) {
        if (st) st[q] = total;
      } else if (en && m <= l) {
        en[l * nl + m] = en[m * nl + l] = total;
      }
    });
    if (tid == 0 && st) {
      st[T] = mx;
      st[T + 1] = barg;
    }
    __syncthreads();  // the next pass writes the reduction rows again
  }
}

// Brhs[cell][m][al][node] of a structured cell: rows m < n_loads = -f^m, the rest zero.  One thread per node: its 6 / 24 incident
// (sub-element, vertex) pairs in the order of K1 (k_assemble_reg), every entry written once
template <int DIM, int KIND>
__global__ __launch_bounds__(128) void k_assemble_loads(int n, LoadOverride lo, long long cell0, const double* __restrict__ Mmat,
                                                        double* __restrict__ Brhs, long long ncells) {
  constexpr KindSizes ks = kind_sizes(DIM, KIND);
  constexpr int T = ks.t, BS = ks.bs, NV = DIM + 1, NSUB = DIM == 2 ? 2 : 6;
  const long long nn = DIM == 2 ? (long long)n * n : (long long)n * n * n, n_el = NSUB * nn;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= ncells * nn) return;
  const long long cell = idx / nn;
  const int node = (int)(idx % nn);
  const int pc[3] = {node % n, (node / n) % n, DIM == 3 ? node / (n * n) : 0};
  double Mp[DIM * DIM];
  cell_M<DIM>(Mmat, cell, Mp);
  const double hn = (double)n;
  const double vol = 1.0 / (DIM == 2 ? 2.0 * hn * hn : 6.0 * hn * hn * hn);
  const double* P = lo.P + (lo.per_cell ? (cell0 + cell) * lo.n_loads : 0) * n_el * T;
  double acc[T][BS];
#pragma unroll
  for (int m = 0; m < T; ++m)
#pragma unroll
    for (int b = 0; b < BS; ++b) acc[m][b] = 0.0;
#pragma unroll
  for (int s = 0; s < NSUB; ++s)
#pragma unroll
    for (int a = 0; a < NV; ++a) {
      int cc[3] = {0, 0, 0};
      double g[DIM];
#pragma unroll
      for (int k = 0; k < DIM; ++k) {
        const int off = DIM == 2 ? kOff2[s][a][k] : kOff3[s][a][k];
        const int v = pc[k] - off;
        cc[k] = v < 0 ? v + n : v;
        g[k] = (DIM == 2 ? kGrad2[s][a][k] : kGrad3[s][a][k]) * hn;
      }
      const long long el = (long long)NSUB * (cc[0] + n * (cc[1] + (long long)n * cc[2])) + s;
#pragma unroll
      for (int b = 0; b < BS; ++b) {
        double sb[T];
        strain<DIM, KIND>(g, Mp, b, sb);
#pragma unroll
        for (int m = 0; m < T; ++m)
          if (m < lo.n_loads) {
            const double* __restrict__ pk = P + ((long long)m * n_el + el) * T;
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < T; ++k) v += pk[k] * sb[k];
            acc[m][b] -= vol * v;
          }
      }
    }
  double* Bc = Brhs + cell * T * BS * nn + node;
#pragma unroll
  for (int m = 0; m < T; ++m)
#pragma unroll
    for (int b = 0; b < BS; ++b) Bc[(long long)(m * BS + b) * nn] = acc[m][b];
}

// the same on a mesh of the tree route: node i gathers through its self-code list (one entry per incident element, ascending), the
// table K1 (k_mesh_assemble) reads its canonical loads through
template <int DIM, int KIND>
__global__ __launch_bounds__(256) void k_assemble_loads_mesh(MeshAsm A, LoadOverride lo, long long cell0, const double* __restrict__ Mall,
                                                             double* __restrict__ Brhs, long long nc) {
  constexpr KindSizes ks = kind_sizes(DIM, KIND);
  constexpr int T = ks.t, BS = ks.bs, NV = DIM + 1;
  const int nn = A.nn;
  const long long total = nc * nn;
  for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += (long long)gridDim.x * blockDim.x) {
    const long long cell = w / nn;
    const int i = (int)(w - cell * nn);
    const double* M = Mall ? Mall + cell * DIM * DIM : nullptr;
    const double* P = lo.P + (lo.per_cell ? (cell0 + cell) * lo.n_loads : 0) * (long long)A.n_el * T;
    const int list = A.self_code[i];
    const int q0 = A.cptr[(long long)list * nn + i], q1 = A.cptr[(long long)list * nn + i + 1];
    double acc[T][BS];
#pragma unroll
    for (int m = 0; m < T; ++m)
#pragma unroll
      for (int b = 0; b < BS; ++b) acc[m][b] = 0.0;
    for (int q = q0; q < q1; ++q) {
      const int ent = A.centry[q], el = ent >> 4, r = (ent >> 2) & 3;
      const double vol = A.vol[el];
      const double* gr = A.grads + ((long long)el * NV + r) * DIM;
#pragma unroll
      for (int b = 0; b < BS; ++b) {
        double sb[T];
        strain<DIM, KIND>(gr, M, b, sb);
#pragma unroll
        for (int m = 0; m < T; ++m)
          if (m < lo.n_loads) {
            const double* __restrict__ pk = P + ((long long)m * A.n_el + el) * T;
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < T; ++k) v += pk[k] * sb[k];
            acc[m][b] -= vol * v;
          }
      }
    }
    double* Bc = Brhs + cell * (long long)T * BS * nn + i;
#pragma unroll
    for (int m = 0; m < T; ++m)
#pragma unroll
      for (int b = 0; b < BS; ++b) Bc[(long long)(m * BS + b) * nn] = acc[m][b];
  }
}

}  // namespace

hipError_t launch_polar(const LoadArgs& a, long long nc, hipStream_t st) {
  return launch_walk(a, nc, st, walk_kernel(a, [](auto D, auto K, auto MESH) { return &k_polar<D(), K(), MESH()>; }));
}

hipError_t launch_load_stats(const LoadArgs& a, long long nc, hipStream_t st) {
  if (a.strain) return launch_walk(a, nc, st, walk_kernel(a, [](auto D, auto K, auto MESH) { return &k_load_stats<D(), K(), MESH(), true>; }));
  return launch_walk(a, nc, st, walk_kernel(a, [](auto D, auto K, auto MESH) { return &k_load_stats<D(), K(), MESH(), false>; }));
}

hipError_t launch_eigenstress(int dim, int kind, const double* coef, const double* E, bool per_cell, double* P, int n_loads, long long n_el,
                              long long nc, hipStream_t st) {
  const long long total = nc * n_loads * n_el;
  if (total <= 0) return hipSuccess;
  return dispatch_dim_kind(dim, kind, [&](auto D, auto K) {
    hipLaunchKernelGGL((k_eigenstress<D(), K()>), dim3(nblk(total)), dim3(256), 0, st, coef, E, per_cell, P, n_loads, n_el, total);
    return hipGetLastError();
  });
}

hipError_t launch_assemble_loads(const BlockedWorkspace* ws, const LoadOverride& lo, long long cell0, const double* Mm, long long nc,
                                 hipStream_t st, double* Brhs) {
  if (nc <= 0) return hipSuccess;
  const Geo& G = ws->G;
  return dispatch_dim_kind(G.dim, G.kind, [&](auto D, auto K) {
    if (ws->mesh_tables) {
      const long long work = nc * (long long)G.nn;
      const unsigned blocks = (unsigned)std::max(1ll, std::min((work + 255) / 256, 1ll << 20));
      hipLaunchKernelGGL((k_assemble_loads_mesh<D(), K()>), dim3(blocks), dim3(256), 0, st, ws->mesh, lo, cell0, Mm, Brhs, nc);
    } else {
      hipLaunchKernelGGL((k_assemble_loads<D(), K()>), dim3(nblk(nc * G.nn, 128)), dim3(128), 0, st, G.n, lo, cell0, Mm, Brhs, nc);
    }
    return hipGetLastError();
  });
}

}  // namespace hommx
