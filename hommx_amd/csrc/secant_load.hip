// secant_load.hip -- one round of the secant iteration beside a load: ONE polarisation or eigenstrain per cell.
//
// Round j of cell c on its current stream cur, whose canonical correctors chi_m and load corrector chi_P the driver has just formed:
//   X    = sum_m xi_m chi_m + chi_P                                           one pass over the correctors, into LDS or the cell's slot
//   e_K  = xi + strain(X)                                                     the total gradient / strain of micro element K
//   polarisation P:  the law reads e_K and q_K = material(cur_K) e_K + P_K    the total flux, as k_criterion forms it
//   eigenstrain E:   the law reads g_K = add_rn(e_K, -E_K), the elastic strain, and q_K = material(cur_K) g_K
//   mean_flux = sum |K| q_K,  strain / flux = what the law read
// and everything else is k_secant_update's round, statement for statement: one body, secant_round (secant_round.h), whose LOAD parts
// are compiled into k_secant_load alone.  History variables are a template parameter; which of P and E is set is decided at run time.
// The tangent beside a load is k_secant_tangent_load's (secant_tangent_load.hip).
//
// One workgroup of kWalkThreads per macro cell, contraction off, fixed-order reductions, no atomics, no inline assembly.
#include <hip/hip_runtime.h>

#include "coef_program.h"
#include "elem_walk.h"
#include "kernels.h"
#include "secant_round.h"
#include "state_program.h"

namespace hommx {

namespace {

template <int DIM, int KIND, bool MESH, bool OUT, bool HIST>
__global__ __launch_bounds__(kWalkThreads) void k_secant_load(SecantLoadArgs A) {
  extern __shared__ double lds_dyn[];
  __shared__ double red[kWalkWaves][kind_sizes(DIM, KIND).t], red_max[kWalkWaves][3];
  secant_round<DIM, KIND, MESH, OUT, HIST, true>(A, lds_dyn, red, red_max, A.hist_in, A.hist_out, A.n_history, A.load);
}

template <bool OUT, bool HIST>
auto round_kernel(const SecantLoadArgs& a) {
  return walk_kernel(a, [](auto D, auto K, auto MESH) { return &k_secant_load<D(), K(), MESH(), OUT, HIST>; });
}

}  // namespace

hipError_t launch_secant_load(const SecantLoadArgs& a, int depth, long long nc, hipStream_t st) {
  if (nc <= 0) return hipSuccess;
  if (depth < 1 || depth > PROGRAM_MAX_STACK || a.round < 0 || a.round >= a.max_iter) return hipErrorInvalidValue;
  if (!a.load.chi || !a.load.P == !a.load.E) return hipErrorInvalidValue;
  const bool hist = a.n_history != 0, out = a.law_values || a.strain;
  if (hist && (a.n_history < 1 || a.n_history > HOMMX_SECANT_MAX_HISTORY || !a.hist_in || !a.hist_out || a.hist_in == a.hist_out))
    return hipErrorInvalidValue;
  const auto kernel = hist ? (out ? round_kernel<true, true>(a) : round_kernel<false, true>(a))
                           : (out ? round_kernel<true, false>(a) : round_kernel<false, false>(a));
  return launch_round(a, kernel, depth, nc, st);
}

}  // namespace hommx
