// fused2d_rhs.hip -- correctors of user-supplied loads on the fused 2D family, by substitution on the factor record (gfx950).
//
// One wavefront per macro cell on the record k_poisson2d_fused<NB, true> left (kernels.h); lane map, signs and index convention of
// fused2d_subst.hip: load case m on a lane bit, column c, KH replicas; N' = -S^-1, y = -x, padding first.  k_fused2d_subst takes the two
// canonical loads, whose forward pass the elimination itself carried (v_j = N'_j r~_j and y_last are in the record).  A general load has to
// make that pass here, so every N'_j is read four times instead of twice:
//     A  forward    r~_0 = r_0,   v_j = N'_j r~_j,   r~_{j+1} = r_{j+1} + E_j v_j                                  (j = 0 .. n-2; v_j kept in LDS)
//     B  backward   g = v_{n-2};  g = v_j + N'_j E_j^T g  (j = n-3 .. 0)          Horner form of sum_j W_j v_j = C g: no arrow block W_j is needed
//        last row   r_last = r_{n-1} + E_{n-2} v_{n-2} + C g,  gauge entry 0,  y_last = N'_last r_last
//     C, D          the u / w sweep and the y sweep of k_fused2d_subst on these v_j and y_last
// and chi_l = -y, mean-free.  C of the text is K[(., n-1), (., 0)]; the record's header holds E_{n-1} = C^T as its two vectors.
//
// The load: K chi_l = -f^l, f^l[i] = sum_{K ni i} |K| P^l_K . M g_a (loads.hip).  The record is of the coefficient scaled by 2^-esh, so
// r = -2^-esh f^l -- M and h enter through f^l alone, esh as an exact power of two -- and x = K'^-1 r is chi_l itself: the M y product of the
// canonical path (whose loads are raw coefficient differences) has no counterpart here.  r_j is formed in the kernel, row by row from the six
// incident (element, vertex) pairs of every node in the order and arithmetic of k_assemble_loads, one row ahead of its use: 12 doubles of P per
// node against the 8 NB doubles of N' the same lane reads per step, no scratch and no second launch, and a shared P stays in cache.
//
// Fixed-order sums, every output entry written once, no atomics, no trip count that depends on data.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "mesh_elem.h"
#include "struct_elem.h"

namespace hommx {

template <int NB>
__global__ __launch_bounds__(64) void k_fused2d_subst_rhs(const double* __restrict__ fact, const double* __restrict__ P, int n_loads,
                                                          long long p_cell_stride, const double* __restrict__ Mmat,
                                                          double* __restrict__ corr, int n, long long ncells) {
  constexpr int NT = NB / 16;
  constexpr int KH = 64 / (2 * NB);  // lanes sharing one (load case, column): 1 (NB = 32), 2 (NB = 16), each sums ROWS rows
  constexpr int ROWS = NB / KH;
  constexpr long long HDR = fused_fact_header(NB), STEP = fused_fact_step(NB);
  __shared__ double ys[NB][2][NB];       // v_j of pass A until pass D overwrites it with y_j
  __shared__ double wsm[NB - 1][2][NB];  // w_j
  __shared__ double vec[2][NB];          // operand of the current product

  const long long cell = blockIdx.x;
  if (cell >= ncells) return;
  __builtin_assume(n >= 3);
  __builtin_assume(n <= NB);
  const int l = threadIdx.x;
  const int c = l % NB, m = (l / NB) & 1, h = l / (2 * NB);
  const int p0 = NB - n;
  const bool valid = c >= p0;
  const int cn = c - p0;                                  // node column
  const int cm = valid ? (c == p0 ? NB - 1 : c - 1) : c;  // cyclic left / right neighbour (matrix index)
  const int cp = valid ? (c == NB - 1 ? p0 : c + 1) : c;
  const int lm = l - c + cm, lp = l - c + cp;             // their lanes in this lane's (load case, replica)
  const double* rec = fact + cell * fused_fact_doubles(n);

  // N'[i][c] of the register-major record: i = 16 ti + 4 r + k, c = 16 tj + jj at ((ti NT + tj) 4 + r) 64 + 16 k + jj
  const int colOff = (c >> 4) * 256 + (c & 15) + h * ROWS * 16;
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

  // ---- the load of node row jr at this lane's (load case, column): -2^-esh f^m, zero on the padding and on the lanes of an absent load ----
  const int esh = (int)rec[4 * NB + 4];
  double Mp[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) Mp[k] = Mmat ? Mmat[cell * 4 + k] : (k % 3 == 0 ? 1.0 : 0.0);
  const double hn = (double)n;
  const double vol = 1.0 / (2.0 * hn * hn);
  const long long n_el = 2ll * n * n;
  const bool loaded = valid && m < n_loads;
  const double* Pm = P + cell * p_cell_stride + (loaded ? m : 0) * n_el * 2;
  auto load_rhs = [&](int jr) {
    double acc = 0.0;
    if (loaded) {
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const int vi = cn - kOff2[s][a][0], vj = jr - kOff2[s][a][1];
          const int ci = vi < 0 ? vi + n : vi, cj = vj < 0 ? vj + n : vj;
          const double g[2] = {kGrad2[s][a][0] * hn, kGrad2[s][a][1] * hn};
          double sb[2];
          strain<2, HOMMX_KIND_POISSON_SCALAR>(g, Mp, 0, sb);
          const double* __restrict__ pk = Pm + (2ll * (ci + n * cj) + s) * 2;
          double v = 0.0;
#pragma unroll
          for (int k = 0; k < 2; ++k) v += pk[k] * sb[k];
          acc -= vol * v;
        }
    }
    return ldexp(acc, -esh);
  };

  double cur[ROWS], nxt[ROWS];
  // ---- A forward: v_j into ys[j]; ends with rt = r_{n-1} + E_{n-2} v_{n-2} and cur = N'_{n-3} ----------------------------------------------
  load_N(rec + HDR, cur);
  double rt = load_rhs(0), g = 0.0;
  for (int j = 0; j <= n - 2; ++j) {
    const double* sp = rec + HDR + j * STEP;
    load_N(j < n - 2 ? sp + STEP : sp - STEP, nxt);  // the block of the next step; of the first step of pass B (n >= 3)
    const double rn = load_rhs(j + 1);
    const double e0 = sp[NB * NB + 2 * NB + c], e1 = sp[NB * NB + 3 * NB + c];
    if (h == 0) vec[m][c] = rt;
    __syncthreads();
    g = matvec(cur);
    __syncthreads();
    if (h == 0) ys[j][m][c] = g;
    rt = rn + mul_E(e0, e1, g);
#pragma unroll
    for (int i = 0; i < ROWS; ++i) cur[i] = nxt[i];
  }
  // ---- B backward (reads only): g = v_j + N'_j E_j^T g; ends with cur = N'_0 and nxt = N'_last --------------------------------------------
  for (int j = n - 3; j >= 0; --j) {
    const double* sp = rec + HDR + j * STEP;
    load_N(j > 0 ? sp - STEP : rec + HDR + (n - 1) * STEP, nxt);
    const double q = mul_ET(sp[NB * NB + 2 * NB + c], sp[NB * NB + 3 * NB + c], g);
    if (h == 0) vec[m][c] = q;
    __syncthreads();
    g = ys[j][m][c] + matvec(cur);
    __syncthreads();
    if (j > 0) {
#pragma unroll
      for (int i = 0; i < ROWS; ++i) cur[i] = nxt[i];
    }
  }
  // ---- last row: y_last = N'_last r_last, the gauged entry (the last index) zero ------------------------------------------------------------
  {
    const double cg = mul_ET(rec[c], rec[NB + c], g);  // every lane takes part in the shuffle
    if (h == 0) vec[m][c] = c == NB - 1 ? 0.0 : rt + cg;
  }
  __syncthreads();
  const double yl = matvec(nxt);
  __syncthreads();

  // ---- C forward: u_j, w_{j+1} (cur holds N'_0) -------------------------------------------------------------------------------------------
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
  // ---- D backward: y_j over v_j in ys[j] (cur holds N'_{n-2}) -----------------------------------------------------------------------------
  if (h == 0) ys[n - 1][m][c] = yl;
  double ynext = yl;
  for (int j = n - 2; j >= 0; --j) {
    const double* sp = rec + HDR + j * STEP;
    if (j > 0) load_N(sp - STEP, nxt);
    const double v = ys[j][m][c];
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

  // ---- chi_l = -y_l, mean-free, dof = i + n j: every entry of the rows l < n_loads written once ------------------------------------------------
  const int nn = n * n;
  double* out = corr + cell * 2ll * nn;
  for (int q = 0; q < n_loads; ++q) {
    double sum = 0.0;
    for (int d = l; d < nn; d += 64) {
      const int jr = d / n, i = d - jr * n + p0;
      sum -= ys[jr][q][i];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
    const double mean = sum / nn;
    for (int d = l; d < nn; d += 64) {
      const int jr = d / n, i = d - jr * n + p0;
      out[q * nn + d] = -ys[jr][q][i] - mean;
    }
  }
}

hipError_t launch_fused2d_subst_rhs(const double* d_fact, const double* d_P, int n_loads, bool per_cell, const double* d_M, double* d_corr, int n,
                                    long long ncells, hipStream_t stream) {
  if (ncells <= 0) return hipSuccess;
  dim3 grid((unsigned)ncells), block(64);
  const long long stride = per_cell ? 4ll * n_loads * n * n : 0;  // doubles of P per cell: [n_loads][2 n n][2]
  if (n <= 16)
    hipLaunchKernelGGL(k_fused2d_subst_rhs<16>, grid, block, 0, stream, d_fact, d_P, n_loads, stride, d_M, d_corr, n, ncells);
  else
    hipLaunchKernelGGL(k_fused2d_subst_rhs<32>, grid, block, 0, stream, d_fact, d_P, n_loads, stride, d_M, d_corr, n, ncells);
  return hipGetLastError();
}

// ---- one step of iterative refinement of the canonical correctors ---------------------------------------------------------------
// The residual of K chi_m = b_m is the load vector of the polarisation field q^m_K = a_K (e_m + M grad chi_m): r = -f(q^m).  So the correction
// is the load corrector of P = q^m on the same record: k_fused2d_subst_rhs with per-cell loads, then chi_m += delta_m (both mean-free).
// One thread per element; q[cell][m][element][2], the layout of P.
__global__ __launch_bounds__(256) void k_fused2d_canonical_flux(const double* __restrict__ coef, const double* __restrict__ Mmat,
                                                                const double* __restrict__ corr, double* __restrict__ q, int n, long long ncells) {
  const long long n_el = 2ll * n * n, nn = (long long)n * n;
  const long long w = blockIdx.x * 256ll + threadIdx.x;
  if (w >= ncells * n_el) return;
  const long long cell = w / n_el;
  const int e = (int)(w - cell * n_el), s = e & 1, ci = (e >> 1) % n, cj = (e >> 1) / n;
  double Mp[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) Mp[k] = Mmat ? Mmat[cell * 4 + k] : (k % 3 == 0 ? 1.0 : 0.0);
  const double hn = (double)n, a = coef[w];
  const double* chi = corr + cell * 2 * nn;
  double sm[2][2] = {{1.0, 0.0}, {0.0, 1.0}};
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    const int ii = ci + kOff2[s][v][0], jj = cj + kOff2[s][v][1];
    const long long node = (ii == n ? 0 : ii) + (long long)n * (jj == n ? 0 : jj);
    const double g[2] = {kGrad2[s][v][0] * hn, kGrad2[s][v][1] * hn};
    double sb[2];
    strain<2, HOMMX_KIND_POISSON_SCALAR>(g, Mp, 0, sb);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const double c = chi[m * nn + node];
      sm[m][0] = fma(c, sb[0], sm[m][0]);
      sm[m][1] = fma(c, sb[1], sm[m][1]);
    }
  }
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    double* out = q + ((cell * 2 + m) * n_el + e) * 2;
    out[0] = a * sm[m][0];
    out[1] = a * sm[m][1];
  }
}

__global__ __launch_bounds__(256) void k_fused2d_add(double* __restrict__ corr, const double* __restrict__ delta, long long total) {
  const long long w = blockIdx.x * 256ll + threadIdx.x;
  if (w < total) corr[w] += delta[w];
}

// d_q: 8 n^2 doubles per cell, d_delta: 2 n^2 doubles per cell (scratch)
hipError_t launch_fused2d_refine(const double* d_fact, const double* d_coef, const double* d_M, double* d_corr, double* d_q, double* d_delta, int n,
                                 long long ncells, hipStream_t stream) {
  if (ncells <= 0) return hipSuccess;
  const long long els = ncells * 2ll * n * n;
  hipLaunchKernelGGL(k_fused2d_canonical_flux, dim3((unsigned)((els + 255) / 256)), dim3(256), 0, stream, d_coef, d_M, d_corr, d_q, n, ncells);
  if (hipError_t e = hipGetLastError()) return e;
  if (hipError_t e = launch_fused2d_subst_rhs(d_fact, d_q, 2, true, d_M, d_delta, n, ncells, stream)) return e;
  hipLaunchKernelGGL(k_fused2d_add, dim3((unsigned)((els + 255) / 256)), dim3(256), 0, stream, d_corr, d_delta, els);
  return hipGetLastError();
}

}  // namespace hommx
