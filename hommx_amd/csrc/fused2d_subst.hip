// fused2d_subst.hip -- correctors of the fused 2D family by substitution on the block inverses k_poisson2d_fused<NB, true> stored (gfx950).
//
// One wavefront per macro cell, pure linear algebra on the cell's factor record (kernels.h): no coefficient, no stencil.  With the signs
// of the elimination (N' = -S^-1, y = -x the solution as the elimination carries it, v_j = N'_j r~_j, E_j = K[(., j+1), (., j)],
// W_j the arrow block of step j, which is never stored):
//     forward in j    w_0 = C^T y_last,   u_j = N'_j w_j,   w_{j+1} = E_j u_j,   w_{n-2} += E_{n-2}^T y_last        (w_j = W_j^T y_last)
//     backward in j   y_j = v_j + N'_j (w_j + E_j^T y_{j+1})                                                       (no E term at j = n-2)
// and chi_m = -(h / 2) sum_k M[m][k] y_k, every load case mean-free.  E and C are bidiagonal: two vectors each (e0[i] = E[i][i],
// e1[i] = E[i][i-1], cyclic on the real indices).
//
// The kernel is bound by reading every N'_j twice.  N' is symmetric, so lane (m, c) forms entry c of N' w_m as sum_i N'[i][c] w_m[i]: for
// a fixed row i the lanes of a load case read one contiguous run of the register-major record, every load of a step is independent of
// the others, and the loads of the next step are issued before the products of the current one.  w_m[i] comes from LDS as a broadcast.
// Index convention as in fused2d.hip: padding first, node column i at matrix index i + NB - n; the padding of every vector is 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace hommx {

template <int NB>
__global__ __launch_bounds__(64) void k_fused2d_subst(const double* __restrict__ fact, double* __restrict__ corr, int n, long long ncells) {
  constexpr int NT = NB / 16;
  constexpr int KH = 64 / (2 * NB);  // lanes sharing one (load case, column): 1 (NB = 32), 2 (NB = 16), each sums ROWS rows
  constexpr int ROWS = NB / KH;
  constexpr long long HDR = fused_fact_header(NB), STEP = fused_fact_step(NB);
  __shared__ double ys[NB][2][NB];       // y of node row j
  __shared__ double wsm[NB - 1][2][NB];  // w_j
  __shared__ double vec[2][NB];          // operand of the current product
  __shared__ double mm[4];

  const long long cell = blockIdx.x;
  if (cell >= ncells) return;
  __builtin_assume(n >= 3);
  __builtin_assume(n <= NB);
  const int l = threadIdx.x;
  const int c = l % NB, m = (l / NB) & 1, h = l / (2 * NB);
  const int p0 = NB - n;
  const bool valid = c >= p0;
  const int cm = valid ? (c == p0 ? NB - 1 : c - 1) : c;  // cyclic left / right neighbour (matrix index)
  const int cp = valid ? (c == NB - 1 ? p0 : c + 1) : c;
  const int lm = l - c + cm, lp = l - c + cp;             // their lanes in this lane's (load case, replica)
  const double* rec = fact + cell * fused_fact_doubles(n);

  // N'[i][c] of the register-major record: i = 16 ti + 4 r + k, c = 16 tj + jj at ((ti NT + tj) 4 + r) 64 + 16 k + jj
  const int colOff = (c >> 4) * 256 + (c & 15) + h * ROWS * 16;  // (NB = 16: rows h ROWS .. of a row-major 16 x 16 matrix)
  auto load_N = [&](const double* sp, double (&nv)[ROWS]) {
#pragma unroll
    for (int i = 0; i < ROWS; ++i) nv[i] = sp[colOff + (i >> 4) * (NT * 256) + ((i >> 2) & 3) * 64 + (i & 3) * 16];
  };
  // entry c of N' vec[m], N' in nv
  auto matvec = [&](const double (&nv)[ROWS]) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < ROWS; ++i) acc[i & 3] = fma(nv[i], vec[m][h * ROWS + i], acc[i & 3]);
    double s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    if (KH == 2) s += __shfl_xor(s, 32, 64);
    return s;
  };
  auto mul_E = [&](double e0, double e1, double y) { return fma(e1, __shfl(y, lm, 64), e0 * y); };    // (E y)[c]
  auto mul_ET = [&](double e0, double e1, double y) { return fma(e0, y, __shfl(e1 * y, lp, 64)); };   // (E^T y)[c]

  const double yl = rec[2 * NB + m * NB + c];
  if (l < 4) mm[l] = rec[4 * NB + l];
  if (h == 0) ys[n - 1][m][c] = yl;

  double cur[ROWS], nxt[ROWS];
  // ---- forward: u_j, w_{j+1} ----------------------------------------------------------------------------------------------
  load_N(rec + HDR, cur);
  double w = mul_E(rec[c], rec[NB + c], yl);
  for (int j = 0; j <= n - 2; ++j) {
    const double* sp = rec + HDR + j * STEP;
    if (j < n - 2) load_N(sp + STEP, nxt);
    const double e0 = sp[NB * NB + 2 * NB + c], e1 = sp[NB * NB + 3 * NB + c];
    if (j == n - 2) w += mul_ET(e0, e1, yl);
    if (h == 0) {
      wsm[j][m][c] = w;
      vec[m][c] = w;
    }
    __syncthreads();
    const double u = matvec(cur);
    __syncthreads();
    w = mul_E(e0, e1, u);
    if (j < n - 2) {
#pragma unroll
      for (int i = 0; i < ROWS; ++i) cur[i] = nxt[i];
    }
  }
  // ---- backward: y_j (cur holds N'_{n-2}) ---------------------------------------------------------------------------------
  double ynext = yl;
  for (int j = n - 2; j >= 0; --j) {
    const double* sp = rec + HDR + j * STEP;
    if (j > 0) load_N(sp - STEP, nxt);
    const double v = sp[NB * NB + m * NB + c];
    double q = wsm[j][m][c];
    if (j < n - 2) q += mul_ET(sp[NB * NB + 2 * NB + c], sp[NB * NB + 3 * NB + c], ynext);
    if (h == 0) vec[m][c] = q;
    __syncthreads();
    ynext = v + matvec(cur);
    __syncthreads();
    if (h == 0) ys[j][m][c] = ynext;
    if (j > 0) {
#pragma unroll
      for (int i = 0; i < ROWS; ++i) cur[i] = nxt[i];
    }
  }
  __syncthreads();

  // ---- chi_m = -(h / 2) (M y)_m, mean-free, dof = i + n j: each corrector written once ----------------------------------------
  const int nn = n * n;
  const double sc = -0.5 / n;
  double* out = corr + cell * 2ll * nn;
  for (int q = 0; q < 2; ++q) {
    const double a0 = sc * mm[2 * q], a1 = sc * mm[2 * q + 1];
    double sum = 0.0;
    for (int d = l; d < nn; d += 64) {
      const int jr = d / n, i = d - jr * n + p0;
      sum += fma(a0, ys[jr][0][i], a1 * ys[jr][1][i]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
    const double mean = sum / nn;
    for (int d = l; d < nn; d += 64) {
      const int jr = d / n, i = d - jr * n + p0;
      out[q * nn + d] = fma(a0, ys[jr][0][i], a1 * ys[jr][1][i]) - mean;
    }
  }
}

hipError_t launch_fused2d_subst(const double* d_fact, double* d_corr, int n, long long ncells, hipStream_t stream) {
  if (ncells <= 0) return hipSuccess;
  dim3 grid((unsigned)ncells), block(64);
  if (n <= 16)
    hipLaunchKernelGGL(k_fused2d_subst<16>, grid, block, 0, stream, d_fact, d_corr, n, ncells);
  else
    hipLaunchKernelGGL(k_fused2d_subst<32>, grid, block, 0, stream, d_fact, d_corr, n, ncells);
  return hipGetLastError();
}

}  // namespace hommx
