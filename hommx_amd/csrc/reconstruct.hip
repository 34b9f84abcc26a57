// reconstruct.hip -- HMM reconstruction of the micro fields inside the sampling boxes.
//
// For macro cell c with macro gradient / strain xi (t entries, canonical-load basis) and the canonical correctors chi_m of the cell:
//   chi^xi = sum_m xi_m chi_m                                            (one pass over the correctors, coalesced over the dof index)
//   s_K    = xi + sum_a sum_alpha chi^xi[p_a bs + alpha] strain(g_a, M, alpha)     reconstructed gradient / strain of micro element K
//   q_K    = material(coef_K) s_K                                        flux A grad R / stress (Voigt order, shear not doubled)
// and the statistics  sum |K| s_K,  sum |K| q_K,  sum |K| s_K . q_K,  max_K |q_K|  and the smallest element reaching it.  The element
// formulas are those of the mesh routes (mesh_elem.h).
//
// One workgroup per macro cell.  chi^xi lives in LDS (or, for cells too large for it, in a per-cell slot of the caller's scratch).
// Statistics: the fixed-order reduction of elem_walk.h (written out in the kernel, see there), so a cell's statistics do not depend on
// its batch position, the chunking or whether fields are written.  No atomics, no inline assembly.
#include <hip/hip_runtime.h>

#include "elem_walk.h"
#include "kernels.h"

namespace hommx {

namespace {

constexpr int kMaxStats = 2 * 6 + 3;

// per-thread running statistics of the elements it visits (ascending element index)
template <int T>
struct Acc {
  double s[T], q[T], e, mx;
  long long arg;
};

// one element: s, q, the optional field rows, and its contribution to the statistics
template <int DIM, int KIND, bool FIELDS>
__device__ __forceinline__ void element(const double (&xi)[KIND >= 2 ? DIM * (DIM + 1) / 2 : DIM], const double* X, const int (&node)[DIM + 1],
                                        const double (&g)[DIM + 1][DIM], double vol, const double* Mc, const double* __restrict__ ce,
                                        long long el, double* __restrict__ srow, double* __restrict__ qrow,
                                        Acc<KIND >= 2 ? DIM * (DIM + 1) / 2 : DIM>& acc) {
  constexpr KindSizes ks = kind_sizes(DIM, KIND);
  constexpr int T = ks.t, BS = ks.bs;
  double s[T];
#pragma unroll
  for (int m = 0; m < T; ++m) s[m] = xi[m];
#pragma unroll
  for (int a = 0; a < DIM + 1; ++a)
#pragma unroll
    for (int al = 0; al < BS; ++al) {
      const double c = X[(long long)node[a] * BS + al];
      double sa[T];
      strain<DIM, KIND>(g[a], Mc, al, sa);
#pragma unroll
      for (int m = 0; m < T; ++m) s[m] += c * sa[m];
    }
  double C[T][T];
  material<DIM, KIND>(ce, C);
  double q[T];
#pragma unroll
  for (int m = 0; m < T; ++m) {
    double v = 0.0;
#pragma unroll
    for (int n = 0; n < T; ++n) v += C[m][n] * s[n];
    q[m] = v;
  }
  if constexpr (FIELDS) {
#pragma unroll
    for (int m = 0; m < T; ++m) {
      srow[m] = s[m];
      qrow[m] = q[m];
    }
  }
  double sq = 0.0, nq = 0.0;
#pragma unroll
  for (int m = 0; m < T; ++m) {
    acc.s[m] += vol * s[m];
    acc.q[m] += vol * q[m];
    sq += s[m] * q[m];
    nq += (KIND >= 2 && m >= DIM ? 2.0 : 1.0) * (q[m] * q[m]);  // Frobenius norm of sigma: shear entries twice
  }
  acc.e += vol * sq;
  const double nrm = sqrt(nq);
  if (nrm > acc.mx) {
    acc.mx = nrm;
    acc.arg = el;
  }
}

// REGIONS (hommx_reconstruct_source with n_regions > 0): 1 + n_regions passes over the elements with one loop body (`pass`).  Pass r = -1
// takes every element: the whole-cell statistics and the fields.  Pass r >= 0 takes the elements labelled r alone -- the label is read
// before the gathers, a skipped element costs one byte --, adds their volumes in one more slot and writes no fields.  Every pass runs the
// same element<>() arithmetic and the same fixed-order reduction, so a region's maximum is bitwise the |q_K| the whole-cell pass saw (as
// the statistics are bitwise the same with and without FIELDS).  Passes, not per-region running sums: eight regions x (2t + 2) sums per
// thread fit neither the registers nor LDS beside chi^xi.
template <int DIM, int KIND, bool MESH, bool FIELDS, bool REGIONS>
__global__ __launch_bounds__(kWalkThreads) void k_recon(ReconArgs A) {
  constexpr KindSizes ks = kind_sizes(DIM, KIND);
  constexpr int T = ks.t, NCOMP = ks.n_comp;
  constexpr int NSUM = 2 * T + 1 + (REGIONS ? 1 : 0);  // sums of a pass: strain, flux, energy (and the volume of a region)
  extern __shared__ double lds_chi[];
  __shared__ double red[kWalkWaves][kMaxStats + (REGIONS ? 1 : 0)];
  const int tid = threadIdx.x;
  const long long cell = blockIdx.x;
  const long long ndof = A.ndof;

  double xi[T];
#pragma unroll
  for (int m = 0; m < T; ++m) xi[m] = A.xi[cell * T + m];
  double Mp[DIM * DIM];
  cell_M<DIM>(A.M, cell, Mp);

  // chi^xi = sum_m xi_m chi_m: every corrector of the cell read once, lanes along the dof index
  double* X = A.slot ? A.slot + cell * ndof : lds_chi;
  const double* corr = A.corr + cell * T * ndof;
  for (long long j = tid; j < ndof; j += kWalkThreads) {
    double v = 0.0;
#pragma unroll
    for (int m = 0; m < T; ++m) v += xi[m] * corr[m * ndof + j];
    X[j] = v;
  }
  __syncthreads();

  const double* cc = A.coef + cell * A.n_el * NCOMP;
  double* srow0 = FIELDS ? A.strain + cell * A.n_el * T : nullptr;
  double* qrow0 = FIELDS ? A.flux + cell * A.n_el * T : nullptr;

  // one pass over the elements and its reduction; W: this pass writes the fields
  auto pass = [&](auto W, const int r) __attribute__((always_inline)) {
    constexpr bool WRITE = FIELDS && decltype(W)::value;
    Acc<T> acc;
#pragma unroll
    for (int m = 0; m < T; ++m) acc.s[m] = acc.q[m] = 0.0;
    acc.e = 0.0;
    acc.mx = -1.0;
    acc.arg = -1;
    double rvol = 0.0;
    for_elements<DIM, MESH>(A, tid, [&](long long el, double vol, auto vertex) {
      if constexpr (REGIONS)
        if (r >= 0 && A.region[el] != r) return;
      int node[DIM + 1];
      double g[DIM + 1][DIM];
#pragma unroll
      for (int a = 0; a < DIM + 1; ++a) vertex(a, node[a], g[a]);
      element<DIM, KIND, WRITE>(xi, X, node, g, vol, Mp, cc + el * NCOMP, el, WRITE ? srow0 + el * T : nullptr,
                                WRITE ? qrow0 + el * T : nullptr, acc);
      if constexpr (REGIONS) rvol += vol;
    });

    // The fixed-order reduction of elem_walk.h, written out here: sums and maximum under one barrier, thread 0 adding wave after wave with
    // every total in registers.  On block_sums / block_argmax the kernel computes the same bits in fewer registers, and 3D elasticity
    // runs 2.5 - 6 % slower for it (the compiler then schedules for an occupancy that the LDS of chi^xi does not allow): DESIGN.md section 3
    double v[NSUM];
#pragma unroll
    for (int m = 0; m < T; ++m) {
      v[m] = acc.s[m];
      v[T + m] = acc.q[m];
    }
    v[2 * T] = acc.e;
    if constexpr (REGIONS) v[2 * T + 1] = rvol;
#pragma unroll
    for (int q = 0; q < NSUM; ++q)
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) v[q] += __shfl_xor(v[q], o, 64);
    double mx = acc.mx;
    long long arg = acc.arg;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const double omx = __shfl_xor(mx, o, 64);
      const long long oarg = __shfl_xor(arg, o, 64);
      if (omx > mx || (omx == mx && oarg < arg && oarg >= 0)) {
        mx = omx;
        arg = oarg;
      }
    }
    const int w = tid >> 6;
    if ((tid & 63) == 0) {
#pragma unroll
      for (int q = 0; q < NSUM; ++q) red[w][q] = v[q];
      red[w][NSUM] = mx;
      red[w][NSUM + 1] = (double)arg;
    }
    __syncthreads();
    if (tid == 0) {
      double t[NSUM];
#pragma unroll
      for (int q = 0; q < NSUM; ++q) t[q] = red[0][q];
      double bmx = red[0][NSUM], barg = red[0][NSUM + 1];
      for (int ww = 1; ww < kWalkWaves; ++ww) {
#pragma unroll
        for (int q = 0; q < NSUM; ++q) t[q] += red[ww][q];
        const double omx = red[ww][NSUM], oarg = red[ww][NSUM + 1];
        if (omx > bmx || (omx == bmx && oarg < barg && oarg >= 0)) {
          bmx = omx;
          barg = oarg;
        }
      }
      // stats[cell] = [the 2t + 1 sums | max | argmax]; a region's row has its volume in front
      double* st = A.stats + cell * (2 * T + 3);
      if constexpr (REGIONS)
        if (r >= 0) {
          st = A.region_stats + (cell * A.n_regions + r) * (2 * T + 4);
          *st++ = t[2 * T + 1];
        }
#pragma unroll
      for (int q = 0; q < 2 * T + 1; ++q) st[q] = t[q];
      st[2 * T + 1] = bmx;
      st[2 * T + 2] = barg;
    }
    if constexpr (REGIONS) __syncthreads();  // the next pass writes the reduction rows again
  };
  pass(std::true_type{}, -1);
  if constexpr (REGIONS)
    for (int r = 0; r < A.n_regions; ++r) pass(std::false_type{}, r);
}

}  // namespace

size_t recon_lds_limit() { return 150 * 1024; }

hipError_t launch_reconstruct(const ReconArgs& a, long long nc, hipStream_t st) {
  if (nc <= 0) return hipSuccess;
  auto with = [&](auto F, auto R) {
    return walk_kernel(a, [](auto D, auto K, auto MESH) { return &k_recon<D(), K(), MESH(), decltype(F)::value, decltype(R)::value>; });
  };
  const bool f = a.strain != nullptr;
  const auto kernel = a.n_regions > 0 ? (f ? with(std::true_type{}, std::true_type{}) : with(std::false_type{}, std::true_type{}))
                                      : (f ? with(std::true_type{}, std::false_type{}) : with(std::false_type{}, std::false_type{}));
  const size_t lds = a.slot ? 0 : sizeof(double) * (size_t)a.ndof;
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  return launch_walk(a, nc, st, kernel, lds);
}

}  // namespace hommx
