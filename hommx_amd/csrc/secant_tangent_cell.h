// secant_tangent_cell.h -- the tangent coefficient of one cell: the one body of k_secant_tangent, k_secant_tangent_history
// (secant_tangent.hip; DESIGN.md sections 4.16, 4.17) and k_secant_tangent_load (secant_load.hip; section 4.18).  The HIST parts are
// compiled into the kernels of a law with history variables alone, the LOAD parts into k_secant_tangent_load alone.
#pragma once
#include <hip/hip_runtime.h>

#include "coef_program.h"
#include "elem_walk.h"
#include "kernels.h"
#include "state_program.h"

namespace hommx {

// position of entry (m, n), m <= n, of the symmetric t x t coefficient in the element stream of the tangent kind: the upper triangle
// row-major (Voigt), or the diagonal first and then 01, 02, 12 (Poisson matrix)
template <int T, bool VOIGT>
__device__ constexpr int tangent_entry(int m, int n) {
  if (VOIGT) return m * T - m * (m - 1) / 2 + (n - m);
  return m == n ? m : T + (m + n - 1);
}

// the widest sweep: all of t = 2 and t = 3 at once; t = 6 in three sweeps of 2 (two sweeps of 3 hold 18 column entries beside the
// interpreter, and the structured Lame instantiation then spills two registers)
constexpr int native_slots(int t) { return t <= 3 ? t : 2; }

// The tangent coefficient of one cell, the body of k_secant_tangent (HIST false: hist_in and n_history are not read) and of
// k_secant_tangent_history, whose law reads h[k] from hist_in[cell][el][n_history]; the program is then the
// law truncated behind the last component's STORE, so every STORE is a component's.  lds_dyn: [the field (ndof), unless it lies in
// the slot | stack[depth - 1][1 + P][kWalkThreads]]; red_max: the reduction rows, the kernel's static LDS
// LOAD: X = sum_m xi_m chi_m + chi_P (chi_P[nc][t][ndof], row 0), and with an eigenstrain E[nc][n_el][t] (null: a polarisation) the
// strain the tangent is evaluated at is the elastic one, add_rn(e_K, -E_K): the strain the law saw in the round
template <int DIM, int KIND, bool MESH, int P, bool HIST, bool LOAD = false>
__device__ __forceinline__ void secant_tangent_cell(const SecantTangentArgs& A, double* lds_dyn, double (*red_max)[2],
                                                    const double* __restrict__ hist_in, int n_history,
                                                    [[maybe_unused]] const double* __restrict__ chi_load = nullptr,
                                                    [[maybe_unused]] const double* __restrict__ E = nullptr) {
#pragma clang fp contract(off)
  constexpr KindSizes ks = kind_sizes(DIM, KIND);
  constexpr int T = ks.t, BS = ks.bs, NCOMP = ks.n_comp, NTAN = T * (T + 1) / 2;
  constexpr bool VOIGT = KIND >= 2;
  static_assert(T % P == 0, "the sweeps tile the t strain entries");
  const int tid = threadIdx.x;
  const long long cell = blockIdx.x;
  const long long ndof = A.ndof;

  double* __restrict__ tan = A.tan + cell * A.n_el * NTAN;
  const double status = A.state[cell * 3 + 2];
  if (!(status == 0.0 || status == 1.0)) {  // no state to linearise at: the identity material
    for (long long i = tid; i < A.n_el * NTAN; i += kWalkThreads) {
      const int q = (int)(i % NTAN);
      bool diag = false;
#pragma unroll
      for (int m = 0; m < T; ++m) diag = diag || q == tangent_entry<T, VOIGT>(m, m);
      tan[i] = diag ? 1.0 : 0.0;
    }
    if (tid == 0) A.asym[cell] = __builtin_nan("");
    return;
  }

  double xi[T];
#pragma unroll
  for (int m = 0; m < T; ++m) xi[m] = A.xi[cell * T + m];
  double Mp[DIM * DIM];
  cell_M<DIM>(A.M, cell, Mp);
  const double* row = A.rows + cell * program_row_doubles(A.n_fields);
  const double x[3] = {row[0], row[1], row[2]};

  // X = sum_m xi_m chi_m (+ chi_P), the statements of k_secant_update / k_secant_load
  double* X = A.slot ? A.slot + cell * ndof : lds_dyn;
  double* stk = (A.slot ? lds_dyn : lds_dyn + ndof) + tid;
  const double* corr = A.corr + cell * T * ndof;
  [[maybe_unused]] const double* chi_P = nullptr;
  if constexpr (LOAD) chi_P = chi_load + cell * T * ndof;
  for (long long j = tid; j < ndof; j += kWalkThreads) {
    double v = 0.0;
#pragma unroll
    for (int m = 0; m < T; ++m) v += xi[m] * corr[m * ndof + j];
    if constexpr (LOAD) v += chi_P[j];
    X[j] = v;
  }
  __syncthreads();

  const long long stream = cell * A.n_el * NCOMP;
  double mx[2] = {0.0, 0.0};  // max |T - T^T|, max |T|
  for_elements<DIM, MESH>(A, tid, [&](long long el, double vol, auto vertex) {
#pragma clang fp contract(off)
    double e[T];
#pragma unroll
    for (int m = 0; m < T; ++m) e[m] = xi[m];
#pragma unroll
    for (int a = 0; a < DIM + 1; ++a) {
      int node;
      double g[DIM];
      vertex(a, node, g);
#pragma unroll
      for (int al = 0; al < BS; ++al) {
        const double c = X[(long long)node * BS + al];
        double sa[T];
        strain<DIM, KIND>(g, Mp, al, sa);
#pragma unroll
        for (int m = 0; m < T; ++m) e[m] += c * sa[m];
      }
    }
    if constexpr (LOAD) {
      if (E) {
#pragma unroll
        for (int m = 0; m < T; ++m) e[m] = add_rn(e[m], -E[(cell * A.n_el + el) * T + m]);
      }
    }
    const double* __restrict__ cu = A.cur + stream + el * NCOMP;
    double* out = tan + el * NTAN;
    double q[T];
#pragma unroll
    for (int m = 0; m < T; ++m) q[m] = 0.0;  // an explicit law reads no s entry (refused on the host): the row holds zeros there
#pragma unroll 1
    for (int off = 0; off < T; off += P) {
      double col[T][P];  // T[m][off + j], from material(cur_K)
#pragma unroll
      for (int m = 0; m < T; ++m)
#pragma unroll
        for (int j = 0; j < P; ++j) col[m][j] = material_entry<DIM, KIND>(cu, m, off + j);
      auto store = [&](int k, double, const double(&d)[P]) {
        double g[T];
        material_column<DIM, KIND>(k, e, g);
#pragma unroll
        for (int m = 0; m < T; ++m)
#pragma unroll
          for (int j = 0; j < P; ++j) col[m][j] = add_rn(col[m][j], mul_rn(g[m], d[j]));
      };
      if constexpr (HIST)
        run_state_program<T, P, true>(A.prog, A.n_fields, x, row, e, q, A.base + stream + el * NCOMP, A.points + el * DIM, stk, store, off,
                                      hist_in + (cell * A.n_el + el) * n_history, NCOMP);
      else
        run_state_program<T, P>(A.prog, A.n_fields, x, row, e, q, A.base + stream + el * NCOMP, A.points + el * DIM, stk, store, off);
      // Column n = off + j against the columns before it.  An entry below the diagonal is parked, raw, in the place of its pair in the
      // stream; when the column of that pair comes -- later in this sweep or in a later one, the same thread either way -- it is read
      // back and the symmetric part takes its place.  col is indexed by constants; what depends on the offset is an address
#pragma unroll
      for (int j = 0; j < P; ++j) {
        const int n = off + j;
#pragma unroll
        for (int m = 0; m < T; ++m) {
          const double v = col[m][j], av = __builtin_fabs(v);
          if (av > mx[1]) mx[1] = av;
          if (m > n) {
            out[tangent_entry<T, VOIGT>(n, m)] = v;
          } else {
            const double w = m == n ? v : out[tangent_entry<T, VOIGT>(m, n)];  // T[n][m]
            out[tangent_entry<T, VOIGT>(m, n)] = mul_rn(0.5, add_rn(v, w));
            const double skew = __builtin_fabs(add_rn(v, -w));
            if (skew > mx[0]) mx[0] = skew;
          }
        }
      }
    }
  });

  block_maxima<2>(mx, red_max, tid);
  if (tid == 0) A.asym[cell] = mx[0] == 0.0 && mx[1] == 0.0 ? 0.0 : div_rn(mx[0], mx[1]);
}

// the launch of `kernel`, the instantiation of `slots` slots per sweep
template <typename Args, typename Kernel>
hipError_t launch_tangent(const Args& a, Kernel kernel, int slots, int depth, long long nc, hipStream_t st) {
  const size_t lds = secant_tangent_lds_bytes(a.slot ? 0 : a.ndof, depth, slots);
  if (lds > recon_lds_limit()) return hipErrorInvalidValue;  // the caller places the field in the slot where it does not fit
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  return launch_walk(a, nc, st, kernel, lds);
}

}  // namespace hommx
