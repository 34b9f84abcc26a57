// secant_tangent.hip -- the coefficient of the consistent tangent of the secant response.
//
// For macro cell c whose secant iteration (secant.hip) has ended with the stream cur and its correctors chi_m, and an EXPLICIT law L
// (one that reads e, c, x, y, p, f but no s), per micro element K:
//   X    = sum_m xi_m chi_m,  e_K = xi + strain(X)                            exactly as k_secant_update forms them
//   T_K  = material(cur_K) + sum_k g_k (dL_k/de)^T,  g_k = material(unit_k) e_K   (material_column, mesh_elem.h)
// accumulated at each STORE k of the forward-mode law as T[m][n] = add_rn(T[m][n], mul_rn(g_k[m], d_k[n])), starting from
// material(cur_K).  The forward mode runs in sweeps of P strain entries (state_program.h); a sweep adds to its own P columns of T, so
// the bits do not depend on P.  Out go the symmetric part mul_rn(0.5, add_rn(T[m][n], T[n][m])) as an element stream of the tangent
// kind -- HOMMX_KIND_POISSON_MATRIX for the Poisson kinds, HOMMX_KIND_ELASTICITY_VOIGT for the elasticity kinds, whose shear
// convention is that of the strain e (doubled), so T needs no scaling -- and per cell asymmetry = max |T - T^T| / max |T| (0 when
// both are 0).  The linear cell problem with that coefficient has A_eff = d sigma_H / d xi.  A cell of status 2 or 3 gets the identity
// material, so that nothing non-finite enters the elimination, and asymmetry NaN.
//
// One workgroup of kWalkThreads per macro cell on elem_walk.h, contraction off, fixed-order maxima, no atomics, no inline assembly.
// Only the t x P columns of the current sweep are live, in registers and indexed by constants; no array of n_comp x t tangents is
// held.  T[m][n] and T[n][m] may come from different sweeps: the lower one waits in the element's own place in the stream.
#include <hip/hip_runtime.h>

#include "coef_program.h"
#include "elem_walk.h"
#include "kernels.h"
#include "secant_tangent_cell.h"
#include "state_program.h"

namespace hommx {

namespace {

template <int DIM, int KIND, bool MESH, int P>
__global__ __launch_bounds__(kWalkThreads) void k_secant_tangent(SecantTangentArgs A) {
  extern __shared__ double lds_dyn[];
  __shared__ double red_max[kWalkWaves][2];
  secant_tangent_cell<DIM, KIND, MESH, P, false>(A, lds_dyn, red_max, nullptr, 0);
}

template <int DIM, int KIND, bool MESH, int P>
__global__ __launch_bounds__(kWalkThreads) void k_secant_tangent_history(SecantTangentHistoryArgs A) {
  extern __shared__ double lds_dyn[];
  __shared__ double red_max[kWalkWaves][2];
  secant_tangent_cell<DIM, KIND, MESH, P, true>(A, lds_dyn, red_max, A.hist_in, A.n_history);
}

__global__ void k_tangent_mask(const double* __restrict__ state, double* __restrict__ tangent, int tt, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  if (state[(i / tt) * 3 + 2] >= 2.0) tangent[i] = __builtin_nan("");
}

}  // namespace

size_t secant_tangent_lds_bytes(long long ndof, int depth, int slots) {
  return sizeof(double) * ((size_t)ndof + (size_t)kWalkThreads * (1 + slots) * (depth - 1));
}

int secant_tangent_slots(int t, int depth) {
  const int native = native_slots(t);
  return secant_tangent_lds_bytes(0, depth, native) <= recon_lds_limit() ? native : 1;
}

hipError_t launch_secant_tangent(const SecantTangentArgs& a, int depth, long long nc, hipStream_t st) {
  if (nc <= 0) return hipSuccess;
  if (depth < 1 || depth > PROGRAM_MAX_STACK) return hipErrorInvalidValue;
  const int slots = secant_tangent_slots(kind_sizes(a.dim, a.kind).t, depth);
  const auto kernel =
      slots > 1 ? walk_kernel(a, [](auto D, auto K, auto MESH) { return &k_secant_tangent<D(), K(), MESH(), native_slots(kind_sizes(D(), K()).t)>; })
                : walk_kernel(a, [](auto D, auto K, auto MESH) { return &k_secant_tangent<D(), K(), MESH(), 1>; });
  return launch_tangent(a, kernel, slots, depth, nc, st);
}

hipError_t launch_secant_tangent_history(const SecantTangentHistoryArgs& a, int depth, long long nc, hipStream_t st) {
  if (nc <= 0) return hipSuccess;
  if (depth < 1 || depth > PROGRAM_MAX_STACK || a.n_history < 1 || a.n_history > HOMMX_SECANT_MAX_HISTORY || !a.hist_in)
    return hipErrorInvalidValue;
  const int slots = secant_tangent_slots(kind_sizes(a.dim, a.kind).t, depth);
  const auto kernel =
      slots > 1 ? walk_kernel(a, [](auto D, auto K, auto MESH) {
        return &k_secant_tangent_history<D(), K(), MESH(), native_slots(kind_sizes(D(), K()).t)>;
      })
                : walk_kernel(a, [](auto D, auto K, auto MESH) { return &k_secant_tangent_history<D(), K(), MESH(), 1>; });
  return launch_tangent(a, kernel, slots, depth, nc, st);
}

hipError_t launch_tangent_mask(const double* state, double* tangent, int tt, long long nc, hipStream_t st) {
  const long long total = nc * tt;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_tangent_mask, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, state, tangent, tt, total);
  return hipGetLastError();
}

}  // namespace hommx
