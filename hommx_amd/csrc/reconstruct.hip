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
// Statistics: element-strided partial sums per thread, a butterfly in each wave, the wave totals in order -- a fixed order, so a cell's
// statistics do not depend on its batch position, the chunking or whether fields are written.  No atomics, no inline assembly.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "mesh_elem.h"
#include "struct_elem.h"

namespace hommx {

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
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
__global__ __launch_bounds__(kThreads) void k_recon(ReconArgs A) {
  constexpr KindSizes ks = kind_sizes(DIM, KIND);
  constexpr int T = ks.t, NCOMP = ks.n_comp;
  constexpr int NSUM = 2 * T + 1 + (REGIONS ? 1 : 0);  // sums of a pass: strain, flux, energy (and the volume of a region)
  extern __shared__ double lds_chi[];
  __shared__ double red[kWaves][kMaxStats + (REGIONS ? 1 : 0)];
  const int tid = threadIdx.x;
  const long long cell = blockIdx.x;
  const long long ndof = A.ndof;

  double xi[T];
#pragma unroll
  for (int m = 0; m < T; ++m) xi[m] = A.xi[cell * T + m];
  // M, or the identity (exact: the same gradients as without M); one private array that never escapes, so it stays in registers
  double Mp[DIM * DIM];
#pragma unroll
  for (int k = 0; k < DIM * DIM; ++k) Mp[k] = A.M ? A.M[cell * DIM * DIM + k] : (k % (DIM + 1) == 0 ? 1.0 : 0.0);

  // chi^xi = sum_m xi_m chi_m: every corrector of the cell read once, lanes along the dof index
  double* X = A.slot ? A.slot + cell * ndof : lds_chi;
  const double* corr = A.corr + cell * T * ndof;
  for (long long j = tid; j < ndof; j += kThreads) {
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

    if constexpr (MESH) {
      for (long long el = tid; el < A.n_el; el += kThreads) {
        if constexpr (REGIONS)
          if (r >= 0 && A.region[el] != r) continue;
        int node[DIM + 1];
        double g[DIM + 1][DIM];
#pragma unroll
        for (int a = 0; a < DIM + 1; ++a) {
          node[a] = A.el_nodes[el * (DIM + 1) + a];
#pragma unroll
          for (int k = 0; k < DIM; ++k) g[a][k] = A.grads[(el * (DIM + 1) + a) * DIM + k];
        }
        const double vol = A.vol[el];
        element<DIM, KIND, WRITE>(xi, X, node, g, vol, Mp, cc + el * NCOMP, el, WRITE ? srow0 + el * T : nullptr,
                                  WRITE ? qrow0 + el * T : nullptr, acc);
        if constexpr (REGIONS) rvol += vol;
      }
    } else {
      // structured: one grid cell (all its sub-simplices, element order n_sub (i + n j [+ n^2 k]) + s) per thread and step
      // (six tetrahedra unrolled hold too many registers: the 3D loop stays rolled, its tables read from constant memory)
      constexpr int NSUB = DIM == 2 ? 2 : 6;
      constexpr int UNROLL = DIM == 2 ? 2 : 1;
      const int n = A.n;
      const double hn = (double)n;
      const long long ncube = A.n_el / NSUB;
      for (long long cube = tid; cube < ncube; cube += kThreads) {
        const int i = (int)(cube % n), j = (int)((cube / n) % n), k = DIM == 3 ? (int)(cube / ((long long)n * n)) : 0;
#pragma unroll UNROLL
        for (int s = 0; s < NSUB; ++s) {
          const long long el = cube * NSUB + s;
          if constexpr (REGIONS)
            if (r >= 0 && A.region[el] != r) continue;
          int node[DIM + 1];
          double g[DIM + 1][DIM];
#pragma unroll
          for (int a = 0; a < DIM + 1; ++a) {
            if constexpr (DIM == 2) {
              const int ii = i + kOff2[s][a][0], jj = j + kOff2[s][a][1];
              node[a] = (ii == n ? 0 : ii) + n * (jj == n ? 0 : jj);
#pragma unroll
              for (int c = 0; c < 2; ++c) g[a][c] = kGrad2[s][a][c] * hn;
            } else {
              const int ii = i + kOff3[s][a][0], jj = j + kOff3[s][a][1], kk = k + kOff3[s][a][2];
              node[a] = (ii == n ? 0 : ii) + n * ((jj == n ? 0 : jj) + n * (kk == n ? 0 : kk));
#pragma unroll
              for (int c = 0; c < 3; ++c) g[a][c] = kGrad3[s][a][c] * hn;
            }
          }
          element<DIM, KIND, WRITE>(xi, X, node, g, A.vol_struct, Mp, cc + el * NCOMP, el, WRITE ? srow0 + el * T : nullptr,
                                    WRITE ? qrow0 + el * T : nullptr, acc);
          if constexpr (REGIONS) rvol += A.vol_struct;
        }
      }
    }

    // fixed-order reduction: wave butterfly, then the wave totals in order
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
      for (int ww = 1; ww < kWaves; ++ww) {
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
    if constexpr (REGIONS) __syncthreads();  // the next pass writes `red` again
  };
  pass(std::true_type{}, -1);
  if constexpr (REGIONS)
    for (int r = 0; r < A.n_regions; ++r) pass(std::false_type{}, r);
}

template <int DIM, int KIND, bool MESH, bool FIELDS, bool REGIONS>
hipError_t launch_one(const ReconArgs& a, long long nc, hipStream_t st) {
  const size_t lds = a.slot ? 0 : sizeof(double) * (size_t)a.ndof;
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)k_recon<DIM, KIND, MESH, FIELDS, REGIONS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((k_recon<DIM, KIND, MESH, FIELDS, REGIONS>), dim3((unsigned)nc), dim3(kThreads), lds, st, a);
  return hipGetLastError();
}

}  // namespace

size_t recon_lds_limit() { return 150 * 1024; }

hipError_t launch_reconstruct(const ReconArgs& a, int dim, int kind, bool mesh, long long nc, hipStream_t st) {
  if (nc <= 0) return hipSuccess;
  const bool f = a.strain != nullptr;
  return dispatch_dim_kind(dim, kind, [&](auto D, auto K) {
    auto with = [&](auto MESH, auto REG) {
      return f ? launch_one<D(), K(), MESH(), true, REG()>(a, nc, st) : launch_one<D(), K(), MESH(), false, REG()>(a, nc, st);
    };
    if (a.n_regions > 0) return mesh ? with(std::true_type{}, std::true_type{}) : with(std::false_type{}, std::true_type{});
    return mesh ? with(std::true_type{}, std::false_type{}) : with(std::false_type{}, std::false_type{});
  });
}

}  // namespace hommx
