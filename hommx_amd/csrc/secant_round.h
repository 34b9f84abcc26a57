// secant_round.h -- the round of one cell of the secant iteration: the one body of k_secant_update, k_secant_history (secant.hip;
// DESIGN.md sections 4.15, 4.17) and k_secant_load (secant_load.hip; section 4.18).  The HIST parts are compiled into the kernels of a
// law with history variables alone, the LOAD parts into k_secant_load alone: an instantiation without them is the code it was.
#pragma once
#include <hip/hip_runtime.h>

#include "coef_program.h"
#include "elem_walk.h"
#include "kernels.h"
#include "state_program.h"

namespace hommx {

// The round of one cell.  lds_dyn: [the field (ndof), unless it lies in the slot | stack[depth - 1][kWalkThreads]]; red, red_max: the
// reduction rows, the kernel's static LDS.
// HIST: the law reads h[k] from hist_in[cell][el][n_history], the history at the start of the call, in every round, and on STORE
// NCOMP + i the update of h[i] goes straight to hist_out[cell][el][i]: no array is held.  A value that is not finite counts towards
// status 2 as a component's does; the history does not enter `change`.  A cell that stops keeps the values of its stopping round, as
// cur does; one that stops with status 2 or 3 gets hist_out = hist_in, bit for bit
// LOAD: X = sum_m xi_m chi_m + chi_P in the same pass over the correctors.  A polarisation: the law sees the total strain e_K and the
// total flux q_K = material(cur_K) e_K + P_K.  An eigenstrain: it sees the elastic strain g_K = add_rn(e_K, -E_K) and
// q_K = material(cur_K) g_K.  mean_flux sums that q_K, and strain / flux are what the law saw
template <int DIM, int KIND, bool MESH, bool OUT, bool HIST, bool LOAD = false>
__device__ __forceinline__ void secant_round(const SecantArgs& A, double* lds_dyn, double (*red)[kind_sizes(DIM, KIND).t], double (*red_max)[3],
                                             const double* __restrict__ hist_in, double* __restrict__ hist_out, int n_history,
                                             [[maybe_unused]] const RoundLoad& L = RoundLoad{}) {
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

  // X = sum_m xi_m chi_m (+ chi_P): every corrector of the cell read once, lanes along the dof index
  double* X = A.slot ? A.slot + cell * ndof : lds_dyn;
  double* stk = (A.slot ? lds_dyn : lds_dyn + ndof) + tid;
  const double* corr = A.corr + cell * T * ndof;
  [[maybe_unused]] const double* chi_P = nullptr;
  if constexpr (LOAD) chi_P = L.chi + cell * T * ndof;
  for (long long j = tid; j < ndof; j += kWalkThreads) {
    double v = 0.0;
#pragma unroll
    for (int m = 0; m < T; ++m) v += xi[m] * corr[m * ndof + j];
    if constexpr (LOAD) v += chi_P[j];
    X[j] = v;
  }
  __syncthreads();

  const long long stream = cell * A.n_el * NCOMP;
  [[maybe_unused]] const double* PE = nullptr;  // LOAD: the cell's P or E rows
  [[maybe_unused]] bool eigen = false;
  if constexpr (LOAD) {
    eigen = L.E != nullptr;
    PE = (eigen ? L.E : L.P) + cell * A.n_el * T;
  }
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
    [[maybe_unused]] double load[T];
    if constexpr (LOAD) {
#pragma unroll
      for (int m = 0; m < T; ++m) load[m] = PE[el * T + m];
      if (eigen) {
#pragma unroll
        for (int m = 0; m < T; ++m) {
          e[m] = add_rn(e[m], -load[m]);  // the elastic strain: what the law and the material see
          load[m] = 0.0;
        }
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
        if constexpr (LOAD) v += load[m];
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

// the launch of a round kernel: dynamic LDS as k_criterion's, with the field in it unless it lies in the slot
template <typename Args, typename Kernel>
hipError_t launch_round(const Args& a, Kernel kernel, int depth, long long nc, hipStream_t st) {
  const size_t lds = criterion_lds_bytes(a.slot ? 0 : a.ndof, depth);
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  return launch_walk(a, nc, st, kernel, lds);
}

}  // namespace hommx
