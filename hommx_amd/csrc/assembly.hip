// assembly.hip -- K1 of the blocked family on structured cells: any dimension (2, 3), any problem kind (scalar / matrix-valued Poisson,
// isotropic / general elasticity), optional stratification matrix M, any n_micro >= 3.
//   k_assemble_reg / k_c0 : periodic P1 stencil (3^d slots x bs x bs per node), canonical loads, C0
//                           (hmm.py:644-650 / 759-772 / 891-903 / 1032-1048; periodic map cell_problem.py:38-300)
// and the device samplers that expand two-phase and separable coefficients into the element stream K1 reads.
//
// Unified element kernel: with w_{a,alpha} in R^t the (Voigt-weighted) "strain" of basis function (a, alpha) and Cv the
// t x t element matrix  E^m : A : E^n :   K = vol w^T Cv w',  B_m = -vol (Cv w)_m,  C0 = sum vol Cv.
// Poisson is the case bs = 1, w_a = M grad(lambda_a), Cv = A (d x d).
#include <hip/hip_runtime.h>


#include <algorithm>
#include <cmath>

#include "blocked_internal.h"
#include "kernels.h"

namespace hommx {

// Voigt weights of sym(e_alpha (x) g): diagonal pairs first, then (01)[,(02),(12)] with factor 2 folded in.  Compile-time (dim, kind) here
// and in the t x t element matrix Cv from the coefficient stream below: everything stays in registers, loops unroll
template <int D, int BSV, int T>
__device__ __forceinline__ void strain_weights_ct(const double* g, int alpha, double* w) {
  if (BSV == 1) {
#pragma unroll
    for (int k = 0; k < D; ++k) w[k] = g[k];
    return;
  }
#pragma unroll
  for (int k = 0; k < D; ++k) w[k] = (k == alpha) ? g[k] : 0.0;
  int m = D;
#pragma unroll
  for (int k = 0; k < D; ++k)
#pragma unroll
    for (int l = k + 1; l < D; ++l, ++m) w[m] = (k == alpha ? g[l] : 0.0) + (l == alpha ? g[k] : 0.0);
}

template <int D, int KIND, int T>
__device__ __forceinline__ void element_matrix_ct(const double* c, double* Cv) {
#pragma unroll
  for (int i = 0; i < T * T; ++i) Cv[i] = 0.0;
  if (KIND == HOMMX_KIND_POISSON_SCALAR) {
#pragma unroll
    for (int k = 0; k < D; ++k) Cv[k * T + k] = c[0];
  } else if (KIND == HOMMX_KIND_POISSON_MATRIX) {
#pragma unroll
    for (int k = 0; k < D; ++k) Cv[k * T + k] = c[k];
    int m = D;
#pragma unroll
    for (int k = 0; k < D; ++k)
#pragma unroll
      for (int l = k + 1; l < D; ++l, ++m) Cv[k * T + l] = Cv[l * T + k] = c[m];
  } else if (KIND == HOMMX_KIND_ELASTICITY_ISO) {
    const double lam = c[0], mu = c[1];
#pragma unroll
    for (int k = 0; k < D; ++k)
#pragma unroll
      for (int l = 0; l < D; ++l) Cv[k * T + l] = lam + (k == l ? 2.0 * mu : 0.0);
#pragma unroll
    for (int m = D; m < T; ++m) Cv[m * T + m] = mu;
  } else {
    int q = 0;
#pragma unroll
    for (int k = 0; k < T; ++k)
#pragma unroll
      for (int l = k; l < T; ++l, ++q) Cv[k * T + l] = Cv[l * T + k] = c[q];
  }
}

// Corner offsets of the sub-elements as compile-time constants (fill_tables() puts the same into Geo::voff): with them the
// stencil slot `code` of every (sub-element, vertex, vertex) triple is a constant and the node's stencil row can stay in registers.
template <int D>
__host__ __device__ constexpr int voff_ct(int s, int a, int k) {
  constexpr int tri[2][3][2] = {{{0, 0}, {1, 0}, {1, 1}}, {{0, 0}, {0, 1}, {1, 1}}};
  constexpr int vb[8][3] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {1, 1, 0}, {0, 0, 1}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1}};
  constexpr int tet[6][4] = {{0, 1, 3, 7}, {0, 1, 7, 5}, {0, 5, 7, 4}, {0, 3, 2, 7}, {0, 6, 4, 7}, {0, 2, 6, 7}};
  return D == 2 ? tri[s][a][k] : vb[tet[s][a]][k];
}
template <int D>
__host__ __device__ constexpr int code_ct(int s, int a, int b) {
  int cd = 0, p3 = 1;
  for (int k = 0; k < D; ++k, p3 *= 3) cd += (voff_ct<D>(s, b, k) - voff_ct<D>(s, a, k) + 1) * p3;
  return cd;
}

// K1 with the node's whole stencil row (NCODE x bs x bs) and load entries accumulated in REGISTERS and written once -- no
// read-modify-write chains through L2, no memset of the stencil array.  Same arithmetic, same order of the 24 / 6 incident
// (sub-element, vertex) pairs as k_assemble: bitwise the same numbers.  ALSPLIT == 0: one thread per node (bs^2 * 3^d <= 36:
// scalar kinds, 2D elasticity); ALSPLIT == 1: one thread per (node, row component) -- 3D elasticity, 81 + 6 accumulators per thread.
template <int D, int KIND, int ALSPLIT>
__global__ __launch_bounds__(128) void k_assemble_reg(Geo G, const double* __restrict__ coef, const double* __restrict__ Mmat,
                                                      double* __restrict__ Kst, double* __restrict__ Brhs, long long ncells) {
  constexpr bool EL = KIND >= HOMMX_KIND_ELASTICITY_ISO;
  constexpr int BSV = EL ? D : 1, T = EL ? D * (D + 1) / 2 : D, NV = D + 1, NSUB = (D == 2) ? 2 : 6, NCODE = (D == 2) ? 9 : 27;
  constexpr int NCOMP = kind_sizes(D, KIND).n_comp;
  constexpr int NAL = ALSPLIT ? 1 : BSV;  // row components per thread
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long nodes = ALSPLIT ? idx / BSV : idx;
  const int al0 = ALSPLIT ? (int)(idx % BSV) : 0;
  if (nodes >= ncells * G.nn) return;
  const long long cell = nodes / G.nn;
  const int node = (int)(nodes % G.nn);
  const int n = G.n;
  int pc[3] = {node % n, (node / n) % n, D == 3 ? node / (n * n) : 0};
  double M[D][D];
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) M[i][j] = Mmat ? Mmat[cell * D * D + i * D + j] : (i == j ? 1.0 : 0.0);
  double vol = 1.0;
#pragma unroll
  for (int k = 0; k < D; ++k) vol /= n;
  vol /= (D == 2 ? 2.0 : 6.0);
  const double* ccell = coef + cell * (long long)G.n_el * NCOMP;
  double Kacc[NCODE * NAL * BSV], Bacc[T * NAL];
#pragma unroll
  for (int i = 0; i < NCODE * NAL * BSV; ++i) Kacc[i] = 0.0;
#pragma unroll
  for (int i = 0; i < T * NAL; ++i) Bacc[i] = 0.0;
#pragma unroll
  for (int s = 0; s < NSUB; ++s) {
#pragma unroll
    for (int a = 0; a < NV; ++a) {
      int cc[3] = {0, 0, 0};
#pragma unroll
      for (int k = 0; k < D; ++k) {
        int v = pc[k] - voff_ct<D>(s, a, k);
        cc[k] = v < 0 ? v + n : v;
      }
      const long long e = (long long)NSUB * (cc[0] + n * (cc[1] + (long long)n * cc[2])) + s;
      double cval[NCOMP];
#pragma unroll
      for (int q = 0; q < NCOMP; ++q) cval[q] = ccell[e * NCOMP + q];
      double Cv[T * T];
      element_matrix_ct<D, KIND, T>(cval, Cv);
      double gt[NV][D];  // g~_b = M (n grad_b)
#pragma unroll
      for (int b = 0; b < NV; ++b)
#pragma unroll
        for (int i = 0; i < D; ++i) {
          double acc = 0.0;
#pragma unroll
          for (int k = 0; k < D; ++k) acc += M[i][k] * G.grad[s][b][k];
          gt[b][i] = acc * n;
        }
#pragma unroll
      for (int ai = 0; ai < NAL; ++ai) {
        const int al = ALSPLIT ? al0 : ai;
        double w[T], y[T];
        strain_weights_ct<D, BSV, T>(gt[a], al, w);
#pragma unroll
        for (int m = 0; m < T; ++m) {
          double acc = 0.0;
#pragma unroll
          for (int q = 0; q < T; ++q) acc += Cv[m * T + q] * w[q];
          y[m] = vol * acc;
        }
#pragma unroll
        for (int m = 0; m < T; ++m) Bacc[m * NAL + ai] -= y[m];
#pragma unroll
        for (int b = 0; b < NV; ++b) {
#pragma unroll
          for (int be = 0; be < BSV; ++be) {
            double wb[T];
            strain_weights_ct<D, BSV, T>(gt[b], be, wb);
            double acc = 0.0;
#pragma unroll
            for (int m = 0; m < T; ++m) acc += y[m] * wb[m];
            Kacc[(code_ct<D>(s, a, b) * NAL + ai) * BSV + be] += acc;
          }
        }
      }
    }
  }
  double* Kc = Kst + cell * (long long)NCODE * BSV * BSV * G.nn;
  double* Bc = Brhs + cell * (long long)T * BSV * G.nn;
#pragma unroll
  for (int code = 0; code < NCODE; ++code)
#pragma unroll
    for (int ai = 0; ai < NAL; ++ai)
#pragma unroll
      for (int be = 0; be < BSV; ++be)
        Kc[(((long long)code * BSV + (ALSPLIT ? al0 : ai)) * BSV + be) * G.nn + node] = Kacc[(code * NAL + ai) * BSV + be];
#pragma unroll
  for (int m = 0; m < T; ++m)
#pragma unroll
    for (int ai = 0; ai < NAL; ++ai) Bc[((long long)m * BSV + (ALSPLIT ? al0 : ai)) * G.nn + node] = Bacc[m * NAL + ai];
}

// C0[cell][t][t] = sum_e vol Cv_e.  Compile-time (dim, kind): the t x t partial sums stay in registers.  WPC waves per macro cell
// (4: one 256-thread block per cell; 1: small meshes, four cells per block, no LDS, no barrier).  Fixed summation order (lane-strided
// partial sums, wave butterfly, wave totals added in order): bitwise reproducible.
template <int D, int KIND, int WPC>
__global__ __launch_bounds__(256) void k_c0(Geo G, const double* __restrict__ coef, double* __restrict__ C0, long long ncells) {
  constexpr bool EL = KIND >= HOMMX_KIND_ELASTICITY_ISO;
  constexpr int T = EL ? D * (D + 1) / 2 : D, TT = T * T;
  constexpr int NCOMP = kind_sizes(D, KIND).n_comp;
  constexpr int NTH = 64 * WPC;  // threads per cell
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long cell = WPC == 4 ? (long long)blockIdx.x : (long long)blockIdx.x * 4 + wave;
  if (cell >= ncells) return;  // WPC == 1: whole waves leave, nothing below synchronises across waves
  double acc[TT];
#pragma unroll
  for (int i = 0; i < TT; ++i) acc[i] = 0.0;
  const double* ccell = coef + cell * (long long)G.n_el * NCOMP;
  for (int e = WPC == 4 ? threadIdx.x : lane; e < G.n_el; e += NTH) {
    double cval[NCOMP], Cv[TT];
#pragma unroll
    for (int q = 0; q < NCOMP; ++q) cval[q] = ccell[(long long)e * NCOMP + q];
    element_matrix_ct<D, KIND, T>(cval, Cv);
#pragma unroll
    for (int i = 0; i < TT; ++i) acc[i] += Cv[i];
  }
  double vol = 1.0;
  for (int k = 0; k < D; ++k) vol /= G.n;
  vol /= (D == 2 ? 2.0 : 6.0);
#pragma unroll
  for (int i = 0; i < TT; ++i) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc[i] += __shfl_xor(acc[i], off, 64);
  }
  if constexpr (WPC == 1) {
#pragma unroll
    for (int i = 0; i < TT; ++i)
      if (lane == i) C0[cell * TT + i] = acc[i] * vol;
  } else {
    __shared__ double red[4][TT];
#pragma unroll
    for (int i = 0; i < TT; ++i)
      if (lane == 0) red[wave][i] = acc[i];
    __syncthreads();
    if (threadIdx.x < TT) C0[cell * TT + threadIdx.x] = (((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x]) * vol;
  }
}

// two-phase media: expand (mask, per-cell phase values) into the element stream the assembly reads
__global__ void k_expand_two_phase(const unsigned char* __restrict__ mask, const double* __restrict__ values,
                                   double* __restrict__ coef, long long n_el, int n_comp, long long ncells) {
  const long long per = n_el * n_comp;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= ncells * per) return;
  const long long cell = idx / per;
  const long long rem = idx % per;
  const long long el = rem / n_comp;
  const int comp = (int)(rem % n_comp);
  coef[idx] = values[(cell * 2 + (mask[el] ? 1 : 0)) * n_comp + comp];
}

hipError_t launch_expand_two_phase(const unsigned char* d_mask, const double* d_values, double* d_coef, long long n_el,
                                   int n_comp, long long ncells, hipStream_t stream) {
  const long long work = ncells * n_el * n_comp;
  if (work <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_expand_two_phase, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, stream, d_mask, d_values, d_coef,
                     n_el, n_comp, ncells);
  return hipGetLastError();
}

// separable coefficients (kernels.h): same arithmetic, operation by operation, as the fused kernel's sampler
__global__ void k_expand_separable(CoefSource src, const double* __restrict__ params, double* __restrict__ coef, long long n_el,
                                   int n_comp, long long ncells) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= ncells * n_el * n_comp) return;
  const int comp = (int)(idx % n_comp);
  const long long el = (idx / n_comp) % n_el, cell = idx / (n_comp * n_el);
  const double a = params[(cell * n_comp + comp) * 2], b = params[(cell * n_comp + comp) * 2 + 1];  // (a, b) of this component
  const double* table = static_cast<const double*>(src.table);
  if (src.mode == COEF_AFFINE) {
    coef[idx] = add_rn(a, mul_rn(b, table[el]));
  } else {
    double acc = 0.0;
    for (int q = 0; q < src.nq; ++q)
      acc = add_rn(acc, mul_rn(src.weights[q], div_rn(1.0, add_rn(a, mul_rn(b, table[el * src.nq + q])))));
    coef[idx] = acc;
  }
}

hipError_t launch_expand_separable(CoefSource src, const double* d_params, double* d_coef, long long n_el, int n_comp, long long ncells,
                                   hipStream_t stream) {
  const long long work = ncells * n_el * n_comp;
  if (work <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_expand_separable, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, stream, src, d_params, d_coef, n_el, n_comp,
                     ncells);
  return hipGetLastError();
}

void fill_tables(Geo& G) {
  const int d = G.dim, nv = d + 1;
  for (int s = 0; s < G.nsub; ++s) {
    double X[4][3] = {};
    for (int a = 0; a < nv; ++a)
      for (int k = 0; k < 3; ++k) {
        int o = 0;
        if (k < d) o = (d == 2) ? voff_ct<2>(s, a, k) : voff_ct<3>(s, a, k);
        G.voff[s][a][k] = o;
        X[a][k] = o;
      }
    // gradients: solve [1 X] coefficients; grad_a = column a of inv([1 X])^T rows 1..d  -> use Cramer via small Gauss-Jordan
    double Aug[4][8] = {};
    for (int a = 0; a < nv; ++a) {
      Aug[a][0] = 1.0;
      for (int k = 0; k < d; ++k) Aug[a][1 + k] = X[a][k];
      Aug[a][nv + a] = 1.0;
    }
    for (int p = 0; p < nv; ++p) {
      int piv = p;
      for (int r = p + 1; r < nv; ++r)
        if (std::fabs(Aug[r][p]) > std::fabs(Aug[piv][p])) piv = r;
      for (int q = 0; q < 2 * nv; ++q) std::swap(Aug[p][q], Aug[piv][q]);
      const double dd = Aug[p][p];
      for (int q = 0; q < 2 * nv; ++q) Aug[p][q] /= dd;
      for (int r = 0; r < nv; ++r)
        if (r != p) {
          const double f = Aug[r][p];
          for (int q = 0; q < 2 * nv; ++q) Aug[r][q] -= f * Aug[p][q];
        }
    }
    // inverse Minv = Aug[:, nv:], lambda_a(x) = Minv[0][a] + sum_k Minv[1+k][a] x_k
    for (int a = 0; a < nv; ++a)
      for (int k = 0; k < 3; ++k) G.grad[s][a][k] = (k < d) ? Aug[1 + k][nv + a] : 0.0;
  }
}

// ---- magnitude normalisation (blocked_internal.h) -------------------------------------------------------------------------------------
// one 256-thread workgroup per cell (grid-stride): largest exponent field of the cell's coefficient stream (wave butterflies, four wave
// maxima through LDS), then the scaled copy.  8 max|coef| |M|_F^2 < 2^esh <= 32 max|coef| |M|_F^2 (exponents of the two factors + 5): the largest stiffness diagonal, sum over the elements of a node
// of vol g~ . C g~, comes out of order one or below in 2D and below in 3D.
__global__ __launch_bounds__(256) void k_coef_normalise(const double* __restrict__ coef, const double* __restrict__ Mall, double* __restrict__ scaled,
                                                        int32_t* __restrict__ esh, long long per_cell, int dim, long long nc) {
  __shared__ int red[4];
  const int tid = threadIdx.x;
  for (long long cell = blockIdx.x; cell < nc; cell += gridDim.x) {
    const double* cc = coef + cell * per_cell;
    int ef = 0;
    for (long long i = tid; i < per_cell; i += 256) ef = max(ef, (__double2hiint(cc[i]) >> 20) & 0x7ff);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) ef = max(ef, __shfl_xor(ef, o, 64));
    if ((tid & 63) == 0) red[tid >> 6] = ef;
    __syncthreads();
    ef = max(max(red[0], red[1]), max(red[2], red[3]));
    double m2 = (double)dim;
    if (Mall) {
      m2 = 0.0;
      for (int i = 0; i < dim * dim; ++i) m2 += Mall[cell * dim * dim + i] * Mall[cell * dim * dim + i];
    }
    const int fm = (__double2hiint(m2) >> 20) & 0x7ff;
    const int sh = (ef == 0 || ef == 0x7ff) ? 0 : (ef - 1023) + (fm == 0 || fm == 0x7ff ? 0 : fm - 1023) + 5;
    double* sc = scaled + cell * per_cell;
    for (long long i = tid; i < per_cell; i += 256) sc[i] = ldexp(cc[i], -sh);
    if (tid == 0) esh[cell] = sh;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_scale_cells(double* __restrict__ buf, long long per_cell, const int32_t* __restrict__ esh, int sign,
                                                     long long nc) {
  const long long total = nc * per_cell;
  for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += (long long)gridDim.x * blockDim.x)
    buf[w] = ldexp(buf[w], sign * esh[w / per_cell]);
}

void launch_coef_normalise(const Geo& G, const double* coef, const double* Mm, long long nc, hipStream_t st, double* scaled, int32_t* esh) {
  if (nc <= 0) return;
  hipLaunchKernelGGL(k_coef_normalise, dim3((unsigned)std::min(nc, 1ll << 20)), dim3(256), 0, st, coef, Mm, scaled, esh,
                     (long long)G.n_el * G.ncomp, G.dim, nc);
}

void launch_scale_cells(double* buf, long long per_cell, const int32_t* esh, int sign, long long nc, hipStream_t st) {
  if (nc <= 0) return;
  hipLaunchKernelGGL(k_scale_cells, dim3((unsigned)std::min((nc * per_cell + 255) / 256, 1ll << 20)), dim3(256), 0, st, buf, per_cell, esh, sign, nc);
}

void launch_assembly(BlockedWorkspace* ws, const double* coef, const double* Mm, long long nc, hipStream_t st, double* Kst, double* Brhs,
                     double* C0) {
  const Geo& G = ws->G;
  dispatch_dim_kind(G.dim, G.kind, [&](auto D, auto K) {
    // ---- K1: the stencil row of a node (3D elasticity: of one row component of a node) in registers, written once, no memset
    constexpr int SPLIT = D() == 3 && K() >= HOMMX_KIND_ELASTICITY_ISO;
    hipLaunchKernelGGL((k_assemble_reg<D(), K(), SPLIT>), dim3(nblk(nc * G.nn * (SPLIT ? D() : 1), 128)), dim3(128), 0, st, G, coef, Mm, Kst,
                       Brhs, nc);
    if (G.n_el <= 4096) hipLaunchKernelGGL((k_c0<D(), K(), 1>), dim3(nblk(nc, 4)), dim3(256), 0, st, G, coef, C0, nc);
    else hipLaunchKernelGGL((k_c0<D(), K(), 4>), dim3((unsigned)nc), dim3(256), 0, st, G, coef, C0, nc);
  });
}

}  // namespace hommx
