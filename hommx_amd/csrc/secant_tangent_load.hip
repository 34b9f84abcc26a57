// secant_tangent_load.hip -- the coefficient of the consistent tangent of the secant response beside a load.
//
// k_secant_tangent_load is k_secant_tangent's cell (secant_tangent_cell.h) with X = sum_m xi_m chi_m + chi_P, the field of the loaded
// round (secant_load.hip), and, beside an eigenstrain, the tangent evaluated at the elastic strain g_K = add_rn(e_K, -E_K):
//   T_K = material(cur_K) + sum_k g_k (dL_k/de)^T,  g_k = material(unit_k) (the strain the law saw)
// An explicit law reads no s entry, so the polarisation itself is not read here.  History variables are a template parameter; whether
// E is set is decided at run time.  Its own translation unit, beside secant_load.hip, so that the build runs the two in parallel.
//
// One workgroup of kWalkThreads per macro cell, contraction off, fixed-order maxima, no atomics, no inline assembly.
#include <hip/hip_runtime.h>

#include "coef_program.h"
#include "elem_walk.h"
#include "kernels.h"
#include "secant_tangent_cell.h"
#include "state_program.h"

namespace hommx {

namespace {

template <int DIM, int KIND, bool MESH, int P, bool HIST>
__global__ __launch_bounds__(kWalkThreads) void k_secant_tangent_load(SecantTangentLoadArgs A) {
  extern __shared__ double lds_dyn[];
  __shared__ double red_max[kWalkWaves][2];
  secant_tangent_cell<DIM, KIND, MESH, P, HIST, true>(A, lds_dyn, red_max, A.hist_in, A.n_history, A.corr_load, A.E);
}

template <bool NATIVE, bool HIST>
auto tangent_kernel(const SecantTangentLoadArgs& a) {
  return walk_kernel(a, [](auto D, auto K, auto MESH) {
    return &k_secant_tangent_load<D(), K(), MESH(), NATIVE ? native_slots(kind_sizes(D(), K()).t) : 1, HIST>;
  });
}

}  // namespace

hipError_t launch_secant_tangent_load(const SecantTangentLoadArgs& a, int depth, long long nc, hipStream_t st) {
  if (nc <= 0) return hipSuccess;
  if (depth < 1 || depth > PROGRAM_MAX_STACK || !a.corr_load) return hipErrorInvalidValue;
  const bool hist = a.n_history != 0;
  if (hist && (a.n_history < 1 || a.n_history > HOMMX_SECANT_MAX_HISTORY || !a.hist_in)) return hipErrorInvalidValue;
  const int slots = secant_tangent_slots(kind_sizes(a.dim, a.kind).t, depth);
  const auto kernel = slots > 1 ? (hist ? tangent_kernel<true, true>(a) : tangent_kernel<true, false>(a))
                                : (hist ? tangent_kernel<false, true>(a) : tangent_kernel<false, false>(a));
  return launch_tangent(a, kernel, slots, depth, nc, st);
}

}  // namespace hommx
