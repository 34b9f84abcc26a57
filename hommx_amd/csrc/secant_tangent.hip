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
#include "state_program.h"

namespace hommx {

namespace {

// position of entry (m, n), m <= n, of the symmetric t x t coefficient in the element stream of the tangent kind: the upper triangle
// row-major (Voigt), or the diagonal first and then 01, 02, 12 (Poisson matrix)
template <int T, bool VOIGT>
__device__ constexpr int tangent_entry(int m, int n) {
  if (VOIGT) return m * T - m * (m - 1) / 2 + (n - m);
  return m == n ? m : T + (m + n - 1);
}

// The tangent coefficient of one cell, the body of k_secant_tangent (HIST false: hist_in and n_history are not read) and of
// k_secant_tangent_history, whose law reads h[k] from hist_in[cell][el][n_history]; the program is then the
// law truncated behind the last component's STORE, so every STORE is a component's.  lds_dyn: [the field (ndof), unless it lies in
// the slot | stack[depth - 1][1 + P][kWalkThreads]]; red_max: the reduction rows, the kernel's static LDS
template <int DIM, int KIND, bool MESH, int P, bool HIST>
__device__ __forceinline__ void secant_tangent_cell(const SecantTangentArgs& A, double* lds_dyn, double (*red_max)[2],
                                                    const double* __restrict__ hist_in, int n_history) {
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

  // X = sum_m xi_m chi_m, the statements of k_secant_update
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

// the widest sweep: all of t = 2 and t = 3 at once; t = 6 in three sweeps of 2 (two sweeps of 3 hold 18 column entries beside the
// interpreter, and the structured Lame instantiation then spills two registers)
constexpr int native_slots(int t) { return t <= 3 ? t : 2; }

}  // namespace

size_t secant_tangent_lds_bytes(long long ndof, int depth, int slots) {
  return sizeof(double) * ((size_t)ndof + (size_t)kWalkThreads * (1 + slots) * (depth - 1));
}

int secant_tangent_slots(int t, int depth) {
  const int native = native_slots(t);
  return secant_tangent_lds_bytes(0, depth, native) <= recon_lds_limit() ? native : 1;
}

namespace {

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

}  // namespace

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
