// criterion_state.hip -- a failure criterion on the NONLINEAR state a secant chunk stopped in.
//
// Behind the last round of a chunk everything the criterion needs is on the device: the current stream cur of every cell, the canonical
// correctors chi_m of the last executed round -- a stopped cell's elimination reproduces them bit for bit -- and, with a load, chi_P
// and the polarisation or the eigenstress of that round; the base stream and history_in.  For macro cell c
//   X    = sum_m xi_m chi_m (+ chi_P)                                         one pass over the correctors, into LDS or the cell's slot
//   e_K  = xi + strain(X)                                                     the total gradient / strain of micro element K
//   q_K  = material(cur_K) e_K (+ P_K)                                        the total flux / stress, P the polarisation or the eigenstress
//   v_K  = program(x, f, e_K, q_K, cur_K, h_K, base_K, y_K)                   ONE scalar, interpreted once per element
// and the statistics of k_criterion.  e_K and q_K are formed statement for statement as k_criterion (criterion.hip) forms them, so for
// a program that reads neither b nor h the result on a given stream, corrector block and load is k_criterion's bit for bit.
//
// One workgroup of kWalkThreads per macro cell on the pieces of elem_walk.h, contraction off, the fixed-order reductions
// block_argmax and block_sums<2>; the stack rows are dynamic LDS sized at launch from the program's validated depth.  Whether a history
// is present is a run-time pointer, uniform over the grid: the interpreter is state_program.h's with both segments compiled in.  No
// atomics, no inline assembly.
#include <hip/hip_runtime.h>

#include "coef_program.h"
#include "elem_walk.h"
#include "kernels.h"
#include "state_program.h"

namespace hommx {

namespace {

template <int DIM, int KIND, bool MESH, bool OUT>
__global__ __launch_bounds__(kWalkThreads) void k_criterion_state(CritStateArgs A) {
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
  const double* bb = A.base + cell * A.n_el * NCOMP;
  const int n_history = A.n_history;
  const double* hh = A.hist_in ? A.hist_in + cell * A.n_el * n_history : nullptr;
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
    run_state_program<T, 0, true, true>(
        A.prog, A.n_fields, x, row, e, q, ce, A.points + el * DIM, stk, [&](int, double value) { v = value; }, 0,
        hh ? hh + el * n_history : nullptr, NCOMP, bb + el * NCOMP, n_history);
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

hipError_t launch_criterion_state(const CritStateArgs& a, int depth, long long nc, hipStream_t st) {
  if (nc <= 0) return hipSuccess;
  if (depth < 1 || depth > PROGRAM_MAX_STACK || a.prog.n_comp != 1 || !a.base) return hipErrorInvalidValue;
  if (a.n_history < 0 || a.n_history > HOMMX_SECANT_MAX_HISTORY || (a.n_history > 0 && !a.hist_in)) return hipErrorInvalidValue;
  const auto kernel = a.values || a.strain
                          ? walk_kernel(a, [](auto D, auto K, auto MESH) { return &k_criterion_state<D(), K(), MESH(), true>; })
                          : walk_kernel(a, [](auto D, auto K, auto MESH) { return &k_criterion_state<D(), K(), MESH(), false>; });
  const size_t lds = criterion_lds_bytes(a.slot ? 0 : a.ndof, depth);
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  return launch_walk(a, nc, st, kernel, lds);
}

}  // namespace hommx
