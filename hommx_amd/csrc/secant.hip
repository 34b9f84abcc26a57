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
// k_secant_history is the same round for a law with history variables: one body, secant_round
// (secant_round.h), whose HIST parts are compiled into that kernel alone.  The round beside a load is k_secant_load's (secant_load.hip).
#include <hip/hip_runtime.h>

#include "coef_program.h"
#include "elem_walk.h"
#include "kernels.h"
#include "secant_round.h"
#include "state_program.h"

namespace hommx {

namespace {

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
