// criterion.hip -- failure criteria evaluated on the reconstructed micro state.
//
// For macro cell c with macro gradient / strain xi, its canonical correctors chi_m and, with a load P, the corrector chi_P of the load:
//   X    = sum_m xi_m chi_m (+ chi_P)                                         one pass over the correctors, into LDS or the cell's slot
//   e_K  = xi + sum_a sum_alpha X[p_a bs + alpha] strain(g_a, M, alpha)       gradient / strain of micro element K (shear doubled)
//   q_K  = material(coef_K) e_K (+ P_K)                                       flux / stress (shear not doubled): k_recon's element<>()
//   v_K  = program(x, f, e_K, q_K, coef_K, y_K)                               the criterion: ONE scalar, interpreted once per element
// and the statistics  max_K v_K  with the smallest element reaching it (a NaN never wins),  sum |K| v_K  (a NaN makes it NaN) and
// sum |K| [v_K >= threshold].  OUT also writes v_K and / or e_K, q_K: the totals the program saw.
//
// One workgroup of kWalkThreads per macro cell on the pieces of elem_walk.h; the reductions are its fixed-order ones, so a cell's
// statistics do not depend on its batch position, the chunking or on OUT.  The whole kernel body is compiled without contraction: which
// products would fuse into an fma depends on the instantiation (with OUT the strain and the flux have one more use), and what the
// program sees must not.
//
// The interpreter is state_program.h's (shared with secant.hip): the program travels by value in the arguments, and its one STORE keeps
// the value.  The stack rows are dynamic LDS sized at launch from the program's validated depth.  No atomics, no inline assembly.
#include <hip/hip_runtime.h>

#include "coef_program.h"
#include "elem_walk.h"
#include "kernels.h"
#include "state_program.h"

namespace hommx {

namespace {

template <int DIM, int KIND, bool MESH, bool OUT>
__global__ __launch_bounds__(kWalkThreads) void k_criterion(CritArgs A) {
#pragma clang fp contract(off)
  constexpr KindSizes ks = kind_sizes(DIM, KIND);
  constexpr int T = ks.t, BS = ks.bs, NCOMP = ks.n_comp;
  extern __shared__ double lds_dyn[];  // [the field (ndof), unless it lies in the slot | stack[depth - 1][kWalkThreads]]
  __shared__ double red[kWalkWaves][2], red_max[kWalkWaves][2];
  const int tid = threadIdx.x;
  const long long cell = blockIdx.x;
  const long long ndof = A.ndof;

  double xi[T];
#pragma unroll
  for (int m = 0; m < T; ++m) xi[m] = A.xi[cell * T + m];
  double Mp[DIM * DIM];
  cell_M<DIM>(A.M, cell, Mp);
  const double* row = A.rows + cell * program_row_doubles(A.n_fields);
  const double x[3] = {row[0], row[1], row[2]};

  // X = sum_m xi_m chi_m (+ chi_P): every corrector of the cell read once, lanes along the dof index
  double* X = A.slot ? A.slot + cell * ndof : lds_dyn;
  double* stk = (A.slot ? lds_dyn : lds_dyn + ndof) + tid;
  const double* corr = A.corr + cell * T * ndof;
  const double* chi_P = A.corr_load ? A.corr_load + cell * T * ndof : nullptr;
  for (long long j = tid; j < ndof; j += kWalkThreads) {
    double v = 0.0;
#pragma unroll
    for (int m = 0; m < T; ++m) v += xi[m] * corr[m * ndof + j];
    if (chi_P) v += chi_P[j];
    X[j] = v;
  }
  __syncthreads();

  const double* cc = A.coef + cell * A.n_el * NCOMP;
  const double* P = A.P ? A.P + (A.per_cell ? cell : 0) * A.n_el * T : nullptr;
  double mx = -__builtin_inf(), sum_v = 0.0, sum_over = 0.0;
  long long arg = -1;
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
    const double* __restrict__ ce = cc + el * NCOMP;
    double q[T];
    {
      double C[T][T];
      material<DIM, KIND>(ce, C);
#pragma unroll
      for (int m = 0; m < T; ++m) {
        double v = 0.0;
#pragma unroll
        for (int n = 0; n < T; ++n) v += C[m][n] * e[n];
        q[m] = P ? v + P[el * T + m] : v;
      }
    }
    double v = 0.0;
    run_state_program<T>(A.prog, A.n_fields, x, row, e, q, ce, A.points + el * DIM, stk, [&](int, double value) { v = value; });
    if constexpr (OUT) {
      if (A.values) A.values[cell * A.n_el + el] = v;
      if (A.strain) {
        double* __restrict__ srow = A.strain + (cell * A.n_el + el) * T;
        double* __restrict__ qrow = A.flux + (cell * A.n_el + el) * T;
#pragma unroll
        for (int m = 0; m < T; ++m) {
          srow[m] = e[m];
          qrow[m] = q[m];
        }
      }
    }
    sum_v += vol * v;
    sum_over += v >= A.threshold ? vol : 0.0;
    if (v > mx) {
      mx = v;
      arg = el;
    }
  });

  double barg = (double)arg;
  block_argmax(mx, barg, red_max, tid);
  double sums[2] = {sum_v, sum_over};
  double* out = A.crit + cell * 4;
  block_sums<2>(sums, red, tid, [&](int q, double total) { out[2 + q] = total; });
  if (tid == 0) {
    out[0] = mx;
    out[1] = barg;
  }
}

}  // namespace

size_t criterion_lds_bytes(long long ndof, int depth) { return sizeof(double) * ((size_t)ndof + (size_t)kWalkThreads * (depth - 1)); }

hipError_t launch_criterion(const CritArgs& a, int depth, long long nc, hipStream_t st) {
  if (nc <= 0) return hipSuccess;
  if (depth < 1 || depth > PROGRAM_MAX_STACK || a.prog.n_comp != 1) return hipErrorInvalidValue;
  const auto kernel = a.values || a.strain ? walk_kernel(a, [](auto D, auto K, auto MESH) { return &k_criterion<D(), K(), MESH(), true>; })
                                           : walk_kernel(a, [](auto D, auto K, auto MESH) { return &k_criterion<D(), K(), MESH(), false>; });
  const size_t lds = criterion_lds_bytes(a.slot ? 0 : a.ndof, depth);
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  return launch_walk(a, nc, st, kernel, lds);
}

}  // namespace hommx
