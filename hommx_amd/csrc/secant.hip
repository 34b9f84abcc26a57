// secant.hip -- one round of the secant (Kacanov) iteration of a strain-dependent coefficient.
//
// For macro cell c with macro gradient / strain xi, the correctors chi_m of its CURRENT element stream cur and its base stream b:
//   X    = sum_m xi_m chi_m                                                   one pass over the correctors, into LDS or the cell's slot
//   e_K  = xi + sum_a sum_alpha X[p_a bs + alpha] strain(g_a, M, alpha)       gradient / strain of micro element K (shear doubled)
//   q_K  = material(cur_K) e_K                                                the secant flux / stress of the current iterate
//   v_K  = program(x, f, e_K, q_K, b_K, y_K)                                  the law: n_comp values, each stored where it is formed
//   w_K  = v_K (relax == 1), else (1 - relax) cur_K + relax v_K               the candidate, two products and one sum, each rounded
// and per cell  change = max |w - cur| / max |w|,  mean_flux = sum |K| q_K.  The workgroup then decides what becomes of the cell
// (hommx_secant_args: the status rules); a cell that goes on copies its candidate into cur in a second pass, a cell that stops leaves
// cur as it is -- the stream A_eff belongs to -- and returns at once in every later round of the chunk.
//
// One workgroup of kWalkThreads per macro cell on the pieces of elem_walk.h; the reductions are its fixed-order ones, no atomics, so a
// cell's outputs do not depend on its batch position, the chunking or on OUT.  The whole kernel body is compiled without contraction,
// as k_criterion's is and for its reason.  The interpreter is state_program.h's; on STORE k the value goes straight to the candidate
// stream, and the running maxima and the non-finite flag are updated there: no array of n_comp values is held.  No inline assembly.
//
// k_secant_history is the same round for a law with history variables: one body, secant_round, whose HIST
// parts are compiled into that kernel alone.
#include <hip/hip_runtime.h>

#include "coef_program.h"
#include "elem_walk.h"
#include "kernels.h"
#include "state_program.h"

namespace hommx {

namespace {

// The round of one cell, the body of k_secant_update (HIST false: hist_in, hist_out and n_history are not read) and of
// k_secant_history.  lds_dyn: [the field (ndof), unless it lies in the slot | stack[depth - 1][kWalkThreads]];
// red, red_max: the reduction rows, the kernel's static LDS.
// HIST: the law reads h[k] from hist_in[cell][el][n_history], the history at the start of the call, in every round, and on STORE
// NCOMP + i the update of h[i] goes straight to hist_out[cell][el][i]: no array is held.  A value that is not finite counts towards
// status 2 as a component's does; the history does not enter `change`.  A cell that stops keeps the values of its stopping round, as
// cur does; one that stops with status 2 or 3 gets hist_out = hist_in, bit for bit
template <int DIM, int KIND, bool MESH, bool OUT, bool HIST>
__device__ __forceinline__ void secant_round(const SecantArgs& A, double* lds_dyn, double (*red)[kind_sizes(DIM, KIND).t], double (*red_max)[3],
                                             const double* __restrict__ hist_in, double* __restrict__ hist_out, int n_history) {
#pragma clang fp contract(off)
  constexpr KindSizes ks = kind_sizes(DIM, KIND);
  constexpr int T = ks.t, BS = ks.bs, NCOMP = ks.n_comp;
  const int tid = threadIdx.x;
  const long long cell = blockIdx.x;
  const long long ndof = A.ndof;

  double* state = A.state + cell * 3;
  if (A.round > 0 && state[2] != -1.0) return;  // the cell has stopped: frozen
  const double rounds = (double)(A.round + 1);
  [[maybe_unused]] const long long hist = cell * A.n_el * n_history;  // HIST: the cell's history rows
  [[maybe_unused]] auto keep_history = [&] {
    for (long long i = tid; i < A.n_el * n_history; i += kWalkThreads) hist_out[hist + i] = hist_in[hist + i];
  };
  if (A.info[cell] != 0) {  // the elimination of this round flagged a pivot: no state to evaluate the law on
    if constexpr (HIST) keep_history();
    if (A.mean_flux && tid < T) A.mean_flux[cell * T + tid] = __builtin_nan("");
    if (tid == 0) {
      state[0] = rounds;
      state[1] = __builtin_nan("");
      state[2] = 3.0;
    }
    return;
  }

  double xi[T];
#pragma unroll
  for (int m = 0; m < T; ++m) xi[m] = A.xi[cell * T + m];
  double Mp[DIM * DIM];
  cell_M<DIM>(A.M, cell, Mp);
  const double* row = A.rows + cell * program_row_doubles(A.n_fields);
  const double x[3] = {row[0], row[1], row[2]};

  // X = sum_m xi_m chi_m: every corrector of the cell read once, lanes along the dof index
  double* X = A.slot ? A.slot + cell * ndof : lds_dyn;
  double* stk = (A.slot ? lds_dyn : lds_dyn + ndof) + tid;
  const double* corr = A.corr + cell * T * ndof;
  for (long long j = tid; j < ndof; j += kWalkThreads) {
    double v = 0.0;
#pragma unroll
    for (int m = 0; m < T; ++m) v += xi[m] * corr[m * ndof + j];
    X[j] = v;
  }
  __syncthreads();

  const long long stream = cell * A.n_el * NCOMP;
  const bool unit = A.relax == 1.0;
  const double keep = 1.0 - A.relax;
  double sums[T], mx[3] = {0.0, 0.0, 0.0};  // sum |K| q_K; max |w - cur|, max |w|, whether some v is not finite
#pragma unroll
  for (int m = 0; m < T; ++m) sums[m] = 0.0;
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
    const double* __restrict__ cu = A.cur + stream + el * NCOMP;
    double q[T];
    {
      double C[T][T];
      material<DIM, KIND>(cu, C);
#pragma unroll
      for (int m = 0; m < T; ++m) {
        double v = 0.0;
#pragma unroll
        for (int n = 0; n < T; ++n) v += C[m][n] * e[n];
        q[m] = v;
        sums[m] += vol * v;
      }
    }
    double* __restrict__ cd = A.cand + stream + el * NCOMP;
    auto store = [&](int k, double v) {
      if constexpr (HIST) {
        if (k >= NCOMP) {  // the update of h[k - NCOMP]
          hist_out[hist + el * n_history + (k - NCOMP)] = v;
          if (!(__builtin_fabs(v) <= 1.7976931348623157e308)) mx[2] = 1.0;
          return;
        }
      }
      const double c = cu[k];
      const double w = unit ? v : add_rn(mul_rn(keep, c), mul_rn(A.relax, v));
      cd[k] = w;
      if constexpr (OUT) {
        if (A.law_values) A.law_values[stream + el * NCOMP + k] = v;
      }
      if (!(__builtin_fabs(v) <= 1.7976931348623157e308)) mx[2] = 1.0;
      const double d = __builtin_fabs(add_rn(w, -c)), aw = __builtin_fabs(w);
      if (d > mx[0]) mx[0] = d;
      if (aw > mx[1]) mx[1] = aw;
    };
    if constexpr (HIST)
      run_state_program<T, 0, true>(A.prog, A.n_fields, x, row, e, q, A.base + stream + el * NCOMP, A.points + el * DIM, stk, store, 0,
                                    hist_in + hist + el * n_history, NCOMP);
    else
      run_state_program<T>(A.prog, A.n_fields, x, row, e, q, A.base + stream + el * NCOMP, A.points + el * DIM, stk, store);
    if constexpr (OUT) {
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
  });

  block_maxima<3>(mx, red_max, tid);  // every thread holds the three totals
  block_sums<T>(sums, red, tid, [&](int q, double total) {
    if (A.mean_flux) A.mean_flux[cell * T + q] = total;
  });
  const double change = mx[0] == 0.0 && mx[1] == 0.0 ? 0.0 : div_rn(mx[0], mx[1]);
  const double status = mx[2] != 0.0 ? 2.0 : change <= A.tol ? 0.0 : A.round + 1 == A.max_iter ? 1.0 : -1.0;
  if (tid == 0) {
    state[0] = rounds;
    state[1] = change;
    state[2] = status;
  }
  if constexpr (HIST) {
    if (status == 2.0) keep_history();  // behind the barriers of the reductions, as the copy below: another thread's stores are done
  }
  if (status != -1.0) return;
  // the cell goes on: the candidate becomes the current stream (the barriers of the reductions lie behind every store to it)
  double* __restrict__ cu = A.cur + stream;
  const double* __restrict__ cd = A.cand + stream;
  for (long long i = tid; i < A.n_el * NCOMP; i += kWalkThreads) cu[i] = cd[i];
}

template <int DIM, int KIND, bool MESH, bool OUT>
__global__ __launch_bounds__(kWalkThreads) void k_secant_update(SecantArgs A) {
  extern __shared__ double lds_dyn[];
  __shared__ double red[kWalkWaves][kind_sizes(DIM, KIND).t], red_max[kWalkWaves][3];
  secant_round<DIM, KIND, MESH, OUT, false>(A, lds_dyn, red, red_max, nullptr, nullptr, 0);
}

template <int DIM, int KIND, bool MESH, bool OUT>
__global__ __launch_bounds__(kWalkThreads) void k_secant_history(SecantHistoryArgs A) {
  extern __shared__ double lds_dyn[];
  __shared__ double red[kWalkWaves][kind_sizes(DIM, KIND).t], red_max[kWalkWaves][3];
  secant_round<DIM, KIND, MESH, OUT, true>(A, lds_dyn, red, red_max, A.hist_in, A.hist_out, A.n_history);
}

}  // namespace

namespace {

template <typename Args, typename Kernel>
hipError_t launch_round(const Args& a, Kernel kernel, int depth, long long nc, hipStream_t st) {
  const size_t lds = criterion_lds_bytes(a.slot ? 0 : a.ndof, depth);
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  return launch_walk(a, nc, st, kernel, lds);
}

}  // namespace

hipError_t launch_secant(const SecantArgs& a, int depth, long long nc, hipStream_t st) {
  if (nc <= 0) return hipSuccess;
  if (depth < 1 || depth > PROGRAM_MAX_STACK || a.round < 0 || a.round >= a.max_iter) return hipErrorInvalidValue;
  const auto kernel = a.law_values || a.strain
                          ? walk_kernel(a, [](auto D, auto K, auto MESH) { return &k_secant_update<D(), K(), MESH(), true>; })
                          : walk_kernel(a, [](auto D, auto K, auto MESH) { return &k_secant_update<D(), K(), MESH(), false>; });
  return launch_round(a, kernel, depth, nc, st);
}

hipError_t launch_secant_history(const SecantHistoryArgs& a, int depth, long long nc, hipStream_t st) {
  if (nc <= 0) return hipSuccess;
  if (depth < 1 || depth > PROGRAM_MAX_STACK || a.round < 0 || a.round >= a.max_iter) return hipErrorInvalidValue;
  if (a.n_history < 1 || a.n_history > HOMMX_SECANT_MAX_HISTORY || !a.hist_in || !a.hist_out || a.hist_in == a.hist_out)
    return hipErrorInvalidValue;
  const auto kernel = a.law_values || a.strain
                          ? walk_kernel(a, [](auto D, auto K, auto MESH) { return &k_secant_history<D(), K(), MESH(), true>; })
                          : walk_kernel(a, [](auto D, auto K, auto MESH) { return &k_secant_history<D(), K(), MESH(), false>; });
  return launch_round(a, kernel, depth, nc, st);
}

}  // namespace hommx
