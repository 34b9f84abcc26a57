// plane.hip -- block-cyclic plane elimination of the periodic micro problem: correctors of plans with small plane blocks (and of fused 2D
// plans), and the route A/B and cross-check runs compare the others against.
//
// Per chunk of macro cells, after K1 (assembly.hip), host-orchestrated batched kernels (grid = cells x tiles):
//   K2  block-cyclic elimination over node planes, block b = bs * n^(d-1) (padded to Bp = 32 k):
//           Sinv = S^-1 (recursive Schur-complement inversion: 32x32 in-register sweeps + fp64-MFMA GEMMs)
//           V = W Sinv ; S_last -= V W^T ; S_next = D_{j+1} - E Sinv E^T ; W_next = -V E^T      (E sparse, from the stencil)
//           Vr = R Sinv ; G += Vr R^T ; R_last -= Vr W^T ; R_next = P_{j+1} - Vr E^T           (t <= 6 load rows, padded to 16)
//   K3  k_finalize : A_H = C0 - G   (== the energy functional hmm.py:652-667 / 774-789 / 905-922 / 1050-1067)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <utility>

#define HOMMX_HIP_TRY_FMT "%s: %s"
#include "blocked_internal.h"
#include "host_common.h"
#include "sweep.h"

namespace hommx {

// ---------------------------------------------------------------------------------------------------------------
// stencil <-> dense plane blocks
// ---------------------------------------------------------------------------------------------------------------

// dst[r][c] += K[(r in plane rowPlane), (c in plane rowPlane + olast)]; optional identity on the padding diagonal
__global__ void k_scatter_plane(Geo G, const double* __restrict__ Kst, double* __restrict__ dst, long long ncells,
                                int rowPlane, int olast, int padIdentity) {
  const int nipc = G.ncode / 3;
  const long long per = (long long)G.Bp * nipc * G.bs;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= ncells * per) return;
  const long long cell = idx / per;
  int rem = (int)(idx % per);
  const int r = rem % G.Bp;
  rem /= G.Bp;
  const int ipc = rem % nipc, be = rem / nipc;
  double* D = dst + cell * (long long)G.Bp * G.Bp;
  if (r >= G.b) {
    if (padIdentity && ipc == 0 && be == 0) D[(long long)r * G.Bp + r] = 1.0;
    return;
  }
  const int q = r / G.bs, al = r % G.bs;
  const int node = q + G.npl * rowPlane;
  const int code = ipc + (olast + 1) * nipc;
  const double v = Kst[((cell * G.ncode + code) * G.bs + al) * G.bs * (long long)G.nn + (long long)be * G.nn + node];
  if (v != 0.0) {
    const int c = plane_neighbour(G, q, ipc) * G.bs + be;
    D[(long long)r * G.Bp + c] += v;
  }
}

// OUT[k][c] (+)= alpha * sum_{k'} IN[k][k'] E[c][k'],  E = K[(., plane rowPlane), (., plane rowPlane + o)]  (OUT = alpha IN E^T);
// o = -1 (codeOff = 0, the elimination) or +1 (codeOff = 2 * 3^(d-1), the back substitution).
// One thread per output column c and tile of RT rows k: the NE = bs * 3^(d-1) entries of E row c and their
// column indices are gathered once into registers and reused for every row of the tile.
// One thread per NODE q (its BSV output columns c = q BSV + al) and tile of RT rows k: the BSV x NE entries of E and
// the NE column indices are gathered once into registers; per row every input IN[k][k'] is loaded once and feeds
// the BSV outputs of the node.
template <int BSV, int NE, int RT>
__global__ __launch_bounds__(256) void k_right_mult_Et(Geo G, const double* __restrict__ Kst,
                                                       const double* __restrict__ IN, double* __restrict__ OUT,
                                                       int nrows, int rowPlane, double alpha, int codeOff,
                                                       int accumulate) {
  const int q = blockIdx.x * 256 + threadIdx.x;  // node in plane (or padding)
  if (q * BSV >= G.Bp) return;
  const long long cell = blockIdx.z;
  const int k0 = blockIdx.y * RT;
  const long long per = (long long)nrows * G.Bp;
  double e[BSV][NE];
  int kx[NE];
  const bool real = q < G.npl;
#pragma unroll
  for (int j = 0; j < NE; ++j) {
    kx[j] = 0;
#pragma unroll
    for (int al = 0; al < BSV; ++al) e[al][j] = 0.0;
  }
  if (real) {
    const int nipc = G.ncode / 3;
    const int node = q + G.npl * rowPlane;
#pragma unroll
    for (int j = 0; j < NE; ++j) {
      const int ipc = j / BSV, be = j % BSV;
      if (ipc < nipc) {
        kx[j] = plane_neighbour(G, q, ipc) * BSV + be;
#pragma unroll
        for (int al = 0; al < BSV; ++al)
          e[al][j] = Kst[((cell * G.ncode + ipc + codeOff) * BSV + al) * BSV * (long long)G.nn + (long long)be * G.nn + node];
      }
    }
  }
  const double* in = IN + cell * per;
  double* out = OUT + cell * per;
  const int k1 = min(nrows, k0 + RT);
  for (int k = k0; k < k1; ++k) {
    const double* row = in + (long long)k * G.Bp;
    double acc[BSV];
#pragma unroll
    for (int al = 0; al < BSV; ++al) acc[al] = 0.0;
#pragma unroll
    for (int j = 0; j < NE; ++j) {
      const double v = row[kx[j]];
#pragma unroll
      for (int al = 0; al < BSV; ++al) acc[al] = fma(v, e[al][j], acc[al]);
    }
#pragma unroll
    for (int al = 0; al < BSV; ++al) {
      const int c = q * BSV + al;
      if (c < G.Bp) {
        double* o = out + (long long)k * G.Bp + c;
        *o = accumulate ? *o + alpha * acc[al] : alpha * acc[al];
      }
    }
  }
}

// OUT[r][c] = alpha * sum_k E[r][k] X[k][c]   (Bp x Bp).  One workgroup per node q (its bs rows r = q bs + al):
// the bs x NE entries of E and the NE row indices are staged in LDS once; every thread then walks its columns c,
// loading each X[k][c] once for the bs output rows.
template <int BSV, int NE>
__global__ __launch_bounds__(256) void k_left_mult_E(Geo G, const double* __restrict__ Kst,
                                                     const double* __restrict__ X, double* __restrict__ OUT,
                                                     int rowPlane, double alpha) {
  __shared__ double es[BSV][NE];
  __shared__ int ks[NE];
  const long long cell = blockIdx.z;
  const int q = blockIdx.x;  // node in plane; rows q*BSV .. q*BSV+BSV-1 ; q >= npl: padding rows
  const long long per = (long long)G.Bp * G.Bp;
  double* out = OUT + cell * per;
  if (q * BSV >= G.b) {  // padding rows: zero
    for (int al = 0; al < BSV; ++al) {
      const int r = q * BSV + al;
      if (r < G.Bp)
        for (int c = threadIdx.x; c < G.Bp; c += 256) out[(long long)r * G.Bp + c] = 0.0;
    }
    return;
  }
  const int nipc = G.ncode / 3;
  if (threadIdx.x < NE) {
    const int j = threadIdx.x, ipc = j / BSV, be = j % BSV;
    const int node = q + G.npl * rowPlane;
    ks[j] = plane_neighbour(G, q, ipc < nipc ? ipc : 0) * BSV + be;
    for (int al = 0; al < BSV; ++al)
      es[al][j] = (ipc < nipc)
                      ? Kst[((cell * G.ncode + ipc) * BSV + al) * BSV * (long long)G.nn + (long long)be * G.nn + node]
                      : 0.0;
  }
  __syncthreads();
  const double* x = X + cell * per;
  for (int c = threadIdx.x; c < G.Bp; c += 256) {
    double acc[BSV];
#pragma unroll
    for (int al = 0; al < BSV; ++al) acc[al] = 0.0;
#pragma unroll
    for (int j = 0; j < NE; ++j) {
      const double xv = x[(long long)ks[j] * G.Bp + c];
#pragma unroll
      for (int al = 0; al < BSV; ++al) acc[al] = fma(es[al][j], xv, acc[al]);
    }
#pragma unroll
    for (int al = 0; al < BSV; ++al) out[(long long)(q * BSV + al) * G.Bp + c] = alpha * acc[al];
  }
}

// XCD-aware ids for the strip kernels: the n workgroups (mesh rows) of one (row block, cell) unit read each other's input segments, so they
// should share an L2, i.e. sit on ONE XCD.  Workgroups go to the XCDs round-robin by linear id: linear id L -> XCD L % 8, mesh row
// (L / 8) % n, unit 8 (L / (8 n)) + L % 8.  (With mesh row = blockIdx.x the n neighbours landed on n different XCDs and every segment was
// fetched from HBM three times.)
__device__ __forceinline__ bool strip_ids(int n, int yblocks, long long nunits, int& jrow, int& by, long long& cell) {
  const unsigned L = blockIdx.x;
  const long long unit = 8ll * (L / (8u * n)) + (L & 7u);
  jrow = (int)((L >> 3) % (unsigned)n);
  if (unit >= nunits) return false;
  by = (int)(unit % yblocks);
  cell = unit / yblocks;
  return true;
}
inline unsigned strip_grid(int n, long long nunits) { return (unsigned)(((nunits + 7) / 8) * 8 * n); }

// Same product for 3D planes with n <= 16: one workgroup per MESH ROW of the plane (n nodes, n BSV output rows) and
// 32-column chunks.  The 3 n BSV input rows the strip depends on (mesh rows j-1, j, j+1) are staged through LDS once
// per chunk -- 3x read amplification instead of the 9x of the node-per-workgroup kernel -- with the next chunk in flight
// in registers; thread (i, cp) owns node i of the strip and columns 2 cp, 2 cp + 1.
template <int BSV>
__global__ __launch_bounds__(256, 3) void k_left_mult_E_strip(Geo G, const double* __restrict__ Kst,
                                                           const double* __restrict__ X, double* __restrict__ OUT,
                                                           int rowPlane, double alpha, long long ncells) {
  constexpr int CW = 32, NN = 9, SLMAX = 16 * BSV, LPT = (SLMAX * CW + 255) / 256;  // loads per thread per segment
  constexpr int NEB = NN * BSV * BSV;
  __shared__ double xs[3][SLMAX][CW];
  __shared__ double es[16][NEB];  // E of the strip's nodes: [node][neighbour][be][al]  (read as 16-lane broadcasts)
  const int tid = threadIdx.x, i = tid >> 4, cp = tid & 15;
  const int n = G.n, SL = n * BSV, Bp = G.Bp;
  int jrow, by_;
  long long cell;
  if (!strip_ids(n, 1, ncells, jrow, by_, cell)) return;
  const long long per = (long long)Bp * Bp;
  const double* x = X + cell * per;
  double* out = OUT + cell * per;
  const bool active = i < n;
  for (int el = tid; el < 16 * NEB; el += 256) {
    const int nd = el / NEB, rem = el % NEB, m = rem / (BSV * BSV), be = (rem / BSV) % BSV, al = rem % BSV;
    double v = 0.0;
    if (nd < n) {
      const int node = nd + n * jrow + G.npl * rowPlane;
      v = Kst[((cell * G.ncode + m) * BSV + al) * BSV * (long long)G.nn + (long long)be * G.nn + node];
    }
    es[nd][rem] = v;
  }
  int lrow[NN];  // LDS row of the neighbour's first component: (oy + 1) * SLMAX + i' * BSV
#pragma unroll
  for (int m = 0; m < NN; ++m) {
    const int ox = m % 3 - 1, oy = m / 3 - 1;
    lrow[m] = active ? (oy + 1) * SLMAX + ((i + ox + n) % n) * BSV : 0;
  }
  int grow[3];  // first global row of the three input segments
#pragma unroll
  for (int sgm = 0; sgm < 3; ++sgm) grow[sgm] = ((jrow + sgm - 1 + n) % n) * SL;
  double g[3][LPT];
  auto fetch = [&](int c0) {
#pragma unroll
    for (int sgm = 0; sgm < 3; ++sgm)
#pragma unroll
      for (int m = 0; m < LPT; ++m) {
        const int el = tid + 256 * m, r = el >> 5, col = el & 31;
        g[sgm][m] = (r < SL) ? x[(long long)(grow[sgm] + r) * Bp + c0 + col] : 0.0;
      }
  };
  auto stash = [&]() {
#pragma unroll
    for (int sgm = 0; sgm < 3; ++sgm)
#pragma unroll
      for (int m = 0; m < LPT; ++m) {
        const int el = tid + 256 * m, r = el >> 5, col = el & 31;
        if (r < SLMAX) xs[sgm][r][col] = g[sgm][m];
      }
  };
  fetch(0);
  for (int c0 = 0; c0 < Bp; c0 += CW) {
    stash();
    __syncthreads();
    if (c0 + CW < Bp) fetch(c0 + CW);
    double acc[BSV][2];
#pragma unroll
    for (int al = 0; al < BSV; ++al) acc[al][0] = acc[al][1] = 0.0;
    int eo = i * NEB;
    asm volatile("" : "+v"(eo));  // keep the E reads in the loop: hoisted they cost 2 NEB VGPRs and a workgroup per CU
    const double* ei = &es[0][0] + eo;
    const double* base = &xs[0][0][0] + 2 * cp;
#pragma unroll
    for (int m = 0; m < NN; ++m) {
#pragma unroll
      for (int be = 0; be < BSV; ++be) {
        const double2 v = *reinterpret_cast<const double2*>(base + (lrow[m] + be) * CW);
#pragma unroll
        for (int al = 0; al < BSV; ++al) {
          const double ev = ei[(m * BSV + be) * BSV + al];
          acc[al][0] = fma(ev, v.x, acc[al][0]);
          acc[al][1] = fma(ev, v.y, acc[al][1]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int al = 0; al < BSV; ++al) {
      acc[al][0] = pin_here(acc[al][0]);
      acc[al][1] = pin_here(acc[al][1]);
    }
    if (active) {
#pragma unroll
      for (int al = 0; al < BSV; ++al)
        *reinterpret_cast<double2*>(out + (long long)((i + n * jrow) * BSV + al) * Bp + c0 + 2 * cp) =
            double2{alpha * acc[al][0], alpha * acc[al][1]};
    }
    __syncthreads();
  }
  if (jrow == 0)  // padding rows b .. Bp-1 of the output are zero
    for (long long idx = (long long)G.b * Bp + tid; idx < per; idx += 256) out[idx] = 0.0;
}

// OUT = alpha IN E^T in the same strip form (the transposed twin of k_left_mult_E_strip): one workgroup per mesh row of
// the plane (its n BSV OUTPUT COLUMNS) and block of rows; 32 rows at a time, the 3 n BSV input columns of each go
// through LDS transposed ([column][row], pitch 34), so the inner loop is the 16 B-read / 16-lane-broadcast loop above.
// E stays in LDS (re-read per chunk: an empty asm hides the loop invariance) to keep 3 workgroups per CU.
template <int BSV>
__global__ __launch_bounds__(256, 2) void k_right_mult_Et_strip(Geo G, const double* __restrict__ Kst,
                                                                const double* __restrict__ IN, double* __restrict__ OUT,
                                                                int nrows, int rowPlane, double alpha, int codeOff,
                                                                int accumulate, int rowsPerBlock, int yblocks, long long ncells) {
  constexpr int CW = 32, CWP = 34, NN = 9, SLMAX = 16 * BSV;
  constexpr int NEB = NN * BSV * BSV;
  __shared__ alignas(16) double xs[3][SLMAX][CWP];
  __shared__ double es[16][NEB];
  __shared__ double ob[CW][SLMAX + 1];
  const int tid = threadIdx.x, i = tid >> 4, rp = tid & 15;
  const int n = G.n, SL = n * BSV, Bp = G.Bp;
  int jrow, by;
  long long cell;
  if (!strip_ids(n, yblocks, (long long)yblocks * ncells, jrow, by, cell)) return;
  const int kbeg = by * rowsPerBlock, kend = min(nrows, kbeg + rowsPerBlock);
  if (kbeg >= kend) return;
  const long long per = (long long)nrows * Bp;
  const double* in = IN + cell * per;
  double* out = OUT + cell * per;
  const bool active = i < n;
  for (int el = tid; el < 16 * NEB; el += 256) {
    const int nd = el / NEB, rem = el % NEB, m = rem / (BSV * BSV), be = (rem / BSV) % BSV, al = rem % BSV;
    double v = 0.0;
    if (nd < n && m < G.ncode / 3) {
      const int node = nd + n * jrow + G.npl * rowPlane;
      v = Kst[((cell * G.ncode + m + codeOff) * BSV + al) * BSV * (long long)G.nn + (long long)be * G.nn + node];
    }
    es[nd][rem] = v;
  }
  int lrow[NN];
#pragma unroll
  for (int m = 0; m < NN; ++m) {
    const int ox = m % 3 - 1, oy = m / 3 - 1;
    lrow[m] = (active ? (oy + 1) * SLMAX + ((i + ox + n) % n) * BSV : 0) * CWP + 2 * rp;
  }
  int gcol[3];  // first global column of the three input segments
#pragma unroll
  for (int sgm = 0; sgm < 3; ++sgm) gcol[sgm] = ((jrow + sgm - 1 + n) % n) * SL;
  const int fr = tid >> 4, fc = tid & 15;  // staging: rows fr, fr + 16 of the chunk, columns fc + 16 m (128 B runs)
  double g[3][2][BSV];
  auto fetch = [&](int k0) {
    // unconditional loads (clamped indices): rows >= kend and columns >= SL land in LDS slots no stored output reads
#pragma unroll
    for (int p2 = 0; p2 < 2; ++p2) {
      const double* src = in + (long long)min(k0 + fr + 16 * p2, kend - 1) * Bp;
#pragma unroll
      for (int sgm = 0; sgm < 3; ++sgm)
#pragma unroll
        for (int m = 0; m < BSV; ++m) g[sgm][p2][m] = src[gcol[sgm] + min(fc + 16 * m, SL - 1)];
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int p2 = 0; p2 < 2; ++p2)
#pragma unroll
      for (int sgm = 0; sgm < 3; ++sgm)
#pragma unroll
        for (int m = 0; m < BSV; ++m) xs[sgm][fc + 16 * m][fr + 16 * p2] = g[sgm][p2][m];
  };
  fetch(kbeg);
  for (int k0 = kbeg; k0 < kend; k0 += CW) {
    stash();
    __syncthreads();
    if (k0 + CW < kend) fetch(k0 + CW);
    double acc[BSV][2];
#pragma unroll
    for (int al = 0; al < BSV; ++al) acc[al][0] = acc[al][1] = 0.0;
    int eo = i * NEB;
    asm volatile("" : "+v"(eo));
    const double* ei = &es[0][0] + eo;
    const double* base = &xs[0][0][0];
#pragma unroll
    for (int m = 0; m < NN; ++m) {
#pragma unroll
      for (int be = 0; be < BSV; ++be) {
        const double2 v = *reinterpret_cast<const double2*>(base + lrow[m] + be * CWP);
#pragma unroll
        for (int al = 0; al < BSV; ++al) {
          const double ev = ei[(m * BSV + be) * BSV + al];
          acc[al][0] = fma(ev, v.x, acc[al][0]);
          acc[al][1] = fma(ev, v.y, acc[al][1]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int al = 0; al < BSV; ++al) {  // the products are final here: do not let them sink into the guarded stores
      acc[al][0] = pin_here(acc[al][0]);
      acc[al][1] = pin_here(acc[al][1]);
    }
    // the 32 x SL output tile leaves through LDS so that the stores run along rows (64 B per 8 lanes) as the loads do
#pragma unroll
    for (int al = 0; al < BSV; ++al) {
      ob[2 * rp][i * BSV + al] = alpha * acc[al][0];
      ob[2 * rp + 1][i * BSV + al] = alpha * acc[al][1];
    }
    __syncthreads();
#pragma unroll
    for (int p2 = 0; p2 < 2; ++p2) {
      const int rr = fr + 16 * p2;
      if (k0 + rr < kend) {
        double* o = out + (long long)(k0 + rr) * Bp + jrow * SL;
#pragma unroll
        for (int m = 0; m < BSV; ++m) {
          const int cc = fc + 16 * m;
          if (cc < SL) o[cc] = accumulate ? o[cc] + ob[rr][cc] : ob[rr][cc];
        }
      }
    }
  }
  if (jrow == 0 && !accumulate)  // padding columns b .. Bp-1 of the output are zero
    for (int k = kbeg; k < kend; ++k)
      for (int cc = G.b + tid; cc < Bp; cc += 256) out[(long long)k * Bp + cc] = 0.0;
}

// R[m][c] (+)= B[m][(c in plane)]  (16 x Bp load rows)
__global__ void k_add_P(Geo G, const double* __restrict__ Brhs, double* __restrict__ R, long long ncells, int plane,
                        int overwrite) {
  const long long per = 16ll * G.Bp;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= ncells * per) return;
  const long long cell = idx / per;
  const int rem = (int)(idx % per);
  const int c = rem % G.Bp, m = rem / G.Bp;
  double v = 0.0;
  if (m < G.t && c < G.b) {
    const int q = c / G.bs, al = c % G.bs;
    v = Brhs[cell * (long long)G.t * G.bs * G.nn + ((long long)m * G.bs + al) * G.nn + q + G.npl * plane];
  }
  if (overwrite) R[idx] = v;
  else R[idx] += v;
}

// gauge: drop the bs unknowns of the last node of the last plane (cell_problem.py:349-361: constants are the kernel)
__global__ void k_pin_last(Geo G, double* __restrict__ Sl, double* __restrict__ Rl, long long ncells) {
  const long long per = (long long)G.Bp * G.bs;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= ncells * per) return;
  const long long cell = idx / per;
  const int rem = (int)(idx % per);
  const int x = rem % G.Bp, p = G.b - G.bs + rem / G.Bp;
  double* S = Sl + cell * (long long)G.Bp * G.Bp;
  S[(long long)p * G.Bp + x] = (x == p) ? 1.0 : 0.0;
  S[(long long)x * G.Bp + p] = (x == p) ? 1.0 : 0.0;
  if (x < 16) Rl[cell * 16ll * G.Bp + (long long)x * G.Bp + p] = 0.0;
}

__global__ void k_finalize(Geo G, const double* __restrict__ C0, const double* __restrict__ Gm, double* __restrict__ out,
                           long long ncells) {
  const int tt = G.t * G.t;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= ncells * tt) return;
  const long long cell = idx / tt;
  const int m = (int)(idx % tt) / G.t, q = (int)(idx % tt) % G.t;
  out[idx] = C0[idx] - Gm[cell * 256 + m * 16 + q];
}

// A[i][j] = A[j][i] for j > i  (mirror the lower triangle; batched, ld = N)
__global__ void k_symmetrize(int N, double* __restrict__ A, long long sA, long long ncells) {
  const long long per = (long long)N * N;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= ncells * per) return;
  const long long cell = idx / per;
  const int rem = (int)(idx % per);
  const int j = rem % N, i = rem / N;
  if (j > i) A[cell * sA + (long long)i * N + j] = A[cell * sA + (long long)j * N + i];
}

// corr[cell][m][plane * b + r] = X[cell][m][r]   (t load cases, periodic dof numbering (node, component))
__global__ void k_store_corr(Geo G, const double* __restrict__ X, double* __restrict__ corr, long long ncells, int plane) {
  const long long per = (long long)G.t * G.b;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= ncells * per) return;
  const long long cell = idx / per;
  const int rem = (int)(idx % per);
  const int r = rem % G.b, m = rem / G.b;
  corr[(cell * G.t + m) * (long long)G.nn * G.bs + (long long)plane * G.b + r] = X[cell * 16ll * G.Bp + (long long)m * G.Bp + r];
}

namespace {
void right_mult_Et(const Ctx& c, const double* Kst, const double* IN, double* OUT, int nrows, int rowPlane, double alpha,
                   int olast = -1, int accumulate = 0) {
  const Geo& G = c.ws->G;
  constexpr int RT = 32;
  const int nodes = (G.Bp + G.bs - 1) / G.bs;
  dim3 grid((nodes + 255) / 256, (nrows + RT - 1) / RT, (unsigned)c.nc), block(256);
  const int ne = G.bs * (G.ncode / 3);
  const int codeOff = (olast + 1) * (G.ncode / 3);
  if (G.dim == 3 && G.n <= 16 && (G.bs == 1 || G.bs == 3)) {  // strip kernel
    int rpb = (nrows + 31) / 32 * 32;  // rows per workgroup: as many as still leave ~4 workgroups per slot
    while (rpb > 32 && (long long)((nrows + rpb - 1) / rpb) * c.nc * G.n < 4096) rpb = (rpb / 2 + 31) / 32 * 32;
    const int yb = (nrows + rpb - 1) / rpb;
    dim3 g2(strip_grid(G.n, (long long)yb * c.nc));
    if (G.bs == 1)
      hipLaunchKernelGGL((k_right_mult_Et_strip<1>), g2, block, 0, c.st, G, Kst, IN, OUT, nrows, rowPlane, alpha, codeOff, accumulate, rpb, yb, c.nc);
    else
      hipLaunchKernelGGL((k_right_mult_Et_strip<3>), g2, block, 0, c.st, G, Kst, IN, OUT, nrows, rowPlane, alpha, codeOff, accumulate, rpb, yb, c.nc);
    return;
  }
#define HOMMX_RM(BSV, NE) hipLaunchKernelGGL((k_right_mult_Et<BSV, NE, RT>), grid, block, 0, c.st, G, Kst, IN, OUT, nrows, rowPlane, alpha, codeOff, accumulate)
  if (ne == 3) HOMMX_RM(1, 3);
  else if (ne == 6) HOMMX_RM(2, 6);
  else if (ne == 9) HOMMX_RM(1, 9);
  else HOMMX_RM(3, 27);
#undef HOMMX_RM
}

void left_mult_E(const Ctx& c, const double* Kst, const double* X, double* OUT, int rowPlane, double alpha) {
  const Geo& G = c.ws->G;
  dim3 grid((G.Bp + G.bs - 1) / G.bs, 1, (unsigned)c.nc), block(256);
  const int ne = G.bs * (G.ncode / 3);
  if (G.dim == 3 && G.n <= 16 && (G.bs == 1 || G.bs == 3)) {  // strip kernel
    dim3 g2(strip_grid(G.n, c.nc));
    if (G.bs == 1) hipLaunchKernelGGL((k_left_mult_E_strip<1>), g2, block, 0, c.st, G, Kst, X, OUT, rowPlane, alpha, c.nc);
    else hipLaunchKernelGGL((k_left_mult_E_strip<3>), g2, block, 0, c.st, G, Kst, X, OUT, rowPlane, alpha, c.nc);
    return;
  }
#define HOMMX_LM(BSV, NE) hipLaunchKernelGGL((k_left_mult_E<BSV, NE>), grid, block, 0, c.st, G, Kst, X, OUT, rowPlane, alpha)
  if (ne == 3) HOMMX_LM(1, 3);
  else if (ne == 6) HOMMX_LM(2, 6);
  else if (ne == 9) HOMMX_LM(1, 9);
  else HOMMX_LM(3, 27);
#undef HOMMX_LM
}

}  // namespace

// The two buffer sets as (pointer, doubles per cell): plane_reserve sizes the chunks by the sum and carves one device block by the list.
struct PlaneBuf {
  double** p;
  long long per_cell;
};

static std::vector<PlaneBuf> main_set(PlaneBufs& pb, const Geo& G) {
  const long long mat = (long long)G.Bp * G.Bp, rows = 16ll * G.Bp;
  return {{&pb.Kst, (long long)G.ncode * G.bs * G.bs * G.nn}, {&pb.Brhs, (long long)G.t * G.bs * G.nn}, {&pb.C0, 36}, {&pb.Cn, (long long)G.n_el * G.ncomp},
          {&pb.EshSlot, 1}, {&pb.S, mat}, {&pb.W, mat},
          {&pb.Sl, mat}, {&pb.V, mat}, {&pb.X, mat}, {&pb.T, mat}, {&pb.R, rows}, {&pb.Rl, rows}, {&pb.Vr, rows}, {&pb.Gm, 256}};
}

static std::vector<PlaneBuf> hist_set(PlaneBufs& pb, const Geo& G) {
  const long long mat = (long long)G.Bp * G.Bp, rows = 16ll * G.Bp;
  return {{&pb.hS, (G.n - 1) * mat}, {&pb.hW, (G.n - 1) * mat}, {&pb.hR, (G.n - 1) * rows}, {&pb.Xa, rows}, {&pb.Xb, rows}, {&pb.Y, rows}};
}

static long long per_cell_bytes(const std::vector<PlaneBuf>& set) {
  long long doubles = 0;
  for (const PlaneBuf& b : set) doubles += b.per_cell;
  return 8 * doubles;
}

static void free_set(void** block, long long* cells, const std::vector<PlaneBuf>& set) {
  if (*block) (void)hipFree(*block);
  *block = nullptr;
  for (const PlaneBuf& b : set) *b.p = nullptr;
  *cells = 0;
}

// one block for `n` cells of every buffer of the set, each at a 256-byte aligned offset; the old block goes first, and a failure leaves the set empty
static int alloc_set(void** block, long long* cells, const std::vector<PlaneBuf>& set, long long n) {
  free_set(block, cells, set);
  std::vector<size_t> off(set.size() + 1, 0);
  for (size_t i = 0; i < set.size(); ++i) off[i + 1] = off[i] + ((size_t)8 * n * set[i].per_cell + 255) / 256 * 256;
  HIP_TRY(hipMalloc(block, off.back()));
  for (size_t i = 0; i < set.size(); ++i) *set[i].p = reinterpret_cast<double*>(static_cast<char*>(*block) + off[i]);
  *cells = n;
  return 0;
}

void plane_free(BlockedWorkspace* ws) {
  PlaneBufs& pb = ws->plane;
  free_set(&pb.block, &pb.chunk, main_set(pb, ws->G));
  free_set(&pb.hblock, &pb.hchunk, hist_set(pb, ws->G));
}

int plane_reserve(BlockedWorkspace* ws, long long ncells, bool correctors) {
  const Geo& G = ws->G;
  PlaneBufs& pb = ws->plane;
  // workspace budget: the batch kernels keep gaining up to ~1000 cells in flight (small launches of the recursive
  // inverse amortise), and the card has 288 GB: take up to 64 GB, never more than half of what is free
  double budget_gb = 64.0;
  {
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess) budget_gb = std::min(budget_gb, 0.5e-9 * (double)fr);
  }
  if (ws->budget_gb_env > 0.0) budget_gb = ws->budget_gb_env;
  const std::vector<PlaneBuf> mset = main_set(pb, G);
  if (correctors) {
    const std::vector<PlaneBuf> hset = hist_set(pb, G);
    long long hc = (long long)(budget_gb * 1e9) / (per_cell_bytes(mset) + per_cell_bytes(hset));
    if (hc < 1) hc = 1;
    if (hc > 8192) hc = 8192;
    if (hc > ncells) hc = ncells;
    if (hc > pb.hchunk)
      if (int rc = alloc_set(&pb.hblock, &pb.hchunk, hset, hc)) return rc;
  }
  long long chunk = (long long)(budget_gb * 1e9) / per_cell_bytes(mset);
  if (chunk < 1) chunk = 1;
  if (chunk > 8192) chunk = 8192;
  if (chunk > ncells) chunk = ncells;
  if (chunk <= pb.chunk) return 0;
  return alloc_set(&pb.block, &pb.chunk, mset, chunk);
}

int plane_eliminate(Ctx c, double* out, double* corr) {
  const PlaneBufs& pb = c.ws->plane;
  const Geo& G = c.ws->G;
  const int n = G.n, Bp = G.Bp;
  const long long mat = (long long)Bp * Bp, nc = c.nc;
  hipStream_t st = c.st;
  // ---- K2 init
  HIP_TRY(hipMemsetAsync(pb.S, 0, 8ll * nc * mat, st));
  HIP_TRY(hipMemsetAsync(pb.W, 0, 8ll * nc * mat, st));
  HIP_TRY(hipMemsetAsync(pb.Sl, 0, 8ll * nc * mat, st));
  HIP_TRY(hipMemsetAsync(pb.Gm, 0, 8ll * nc * 256, st));
  const long long scat = nc * (long long)Bp * (G.ncode / 3) * G.bs;
  hipLaunchKernelGGL(k_scatter_plane, dim3(nblk(scat)), dim3(256), 0, st, G, pb.Kst, pb.S, nc, 0, 0, 1);
  hipLaunchKernelGGL(k_scatter_plane, dim3(nblk(scat)), dim3(256), 0, st, G, pb.Kst, pb.W, nc, n - 1, +1, 0);
  hipLaunchKernelGGL(k_scatter_plane, dim3(nblk(scat)), dim3(256), 0, st, G, pb.Kst, pb.Sl, nc, n - 1, 0, 1);
  hipLaunchKernelGGL(k_add_P, dim3(nblk(nc * 16ll * Bp)), dim3(256), 0, st, G, pb.Brhs, pb.R, nc, 0, 1);
  hipLaunchKernelGGL(k_add_P, dim3(nblk(nc * 16ll * Bp)), dim3(256), 0, st, G, pb.Brhs, pb.Rl, nc, n - 1, 1);
  // ---- K2 elimination of planes 0 .. n-2
  for (int j = 0; j <= n - 2; ++j) {
    const bool last = (j == n - 2);
    c.stepcode = j + 1;
    if (last)  // the last plane couples to plane n-2 through E as well as through the arrow
      hipLaunchKernelGGL(k_scatter_plane, dim3(nblk(scat)), dim3(256), 0, st, G, pb.Kst, pb.W, nc, n - 1, -1, 0);
    invert(c, pb.S, 0, Bp, pb.T);                                                                   // S <- S^-1
    if (corr) {  // keep what the back substitution needs: S_j^-1, W_j (incl. E on the last step), R_j
      HIP_TRY(hipMemcpyAsync(pb.hS + (long long)j * nc * mat, pb.S, 8ll * nc * mat, hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemcpyAsync(pb.hW + (long long)j * nc * mat, pb.W, 8ll * nc * mat, hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemcpyAsync(pb.hR + (long long)j * nc * 16 * Bp, pb.R, 8ll * nc * 16 * Bp, hipMemcpyDeviceToDevice, st));
    }
    gemm(c, false, false, Bp, Bp, Bp, 1.0, pb.W, Bp, mat, pb.S, Bp, mat, 0.0, pb.V, Bp, mat);      // V = W Sinv
    gemm(c, false, true, Bp, Bp, Bp, -1.0, pb.V, Bp, mat, pb.W, Bp, mat, 1.0, pb.Sl, Bp, mat, 1);  // S_last -= V W^T (lower tiles)
    gemm(c, false, false, 16, Bp, Bp, 1.0, pb.R, Bp, 16ll * Bp, pb.S, Bp, mat, 0.0, pb.Vr, Bp, 16ll * Bp);   // Vr = R Sinv
    gemm(c, false, true, 16, 16, Bp, 1.0, pb.Vr, Bp, 16ll * Bp, pb.R, Bp, 16ll * Bp, 1.0, pb.Gm, 16, 256);   // G += Vr R^T
    gemm(c, false, true, 16, Bp, Bp, -1.0, pb.Vr, Bp, 16ll * Bp, pb.W, Bp, mat, 1.0, pb.Rl, Bp, 16ll * Bp);  // R_last -= Vr W^T
    if (!last) {
      right_mult_Et(c, pb.Kst, pb.S, pb.X, Bp, j + 1, 1.0);   // X = Sinv E^T
      left_mult_E(c, pb.Kst, pb.X, pb.S, j + 1, -1.0);        // S = -E X
      hipLaunchKernelGGL(k_scatter_plane, dim3(nblk(scat)), dim3(256), 0, st, G, pb.Kst, pb.S, nc, j + 1, 0, 1);                 // S += D_{j+1}
      right_mult_Et(c, pb.Kst, pb.V, pb.W, Bp, j + 1, -1.0);  // W = -V E^T
      right_mult_Et(c, pb.Kst, pb.Vr, pb.R, 16, j + 1, -1.0);  // R = -Vr E^T
      hipLaunchKernelGGL(k_add_P, dim3(nblk(nc * 16ll * Bp)), dim3(256), 0, st, G, pb.Brhs, pb.R, nc, j + 1, 0);                 // R += P_{j+1}
    }
  }
  // ---- last plane
  c.stepcode = n;
  hipLaunchKernelGGL(k_symmetrize, dim3(nblk(nc * mat)), dim3(256), 0, st, Bp, pb.Sl, mat, nc);  // mirror the lower tiles
  hipLaunchKernelGGL(k_pin_last, dim3(nblk(nc * (long long)Bp * G.bs)), dim3(256), 0, st, G, pb.Sl, pb.Rl, nc);
  invert(c, pb.Sl, 0, Bp, pb.T);
  gemm(c, false, false, 16, Bp, Bp, 1.0, pb.Rl, Bp, 16ll * Bp, pb.Sl, Bp, mat, 0.0, pb.Vr, Bp, 16ll * Bp);
  gemm(c, false, true, 16, 16, Bp, 1.0, pb.Vr, Bp, 16ll * Bp, pb.Rl, Bp, 16ll * Bp, 1.0, pb.Gm, 16, 256);
  // ---- correctors: back substitution  chi_j = S_j^-1 (r_j - E_j^T chi_{j+1} - W_j^T chi_last), rows = load cases
  if (corr) {
    const long long sx = 16ll * Bp;
    hipLaunchKernelGGL(k_store_corr, dim3(nblk(nc * (long long)G.t * G.b)), dim3(256), 0, st, G, pb.Vr, corr, nc, n - 1);
    double* Xn = pb.Xa;  // chi_{j+1}
    double* Xc = pb.Xb;  // chi_j
    for (int j = n - 2; j >= 0; --j) {
      HIP_TRY(hipMemcpyAsync(pb.Y, pb.hR + (long long)j * nc * sx, 8ll * nc * sx, hipMemcpyDeviceToDevice, st));
      gemm(c, false, false, 16, Bp, Bp, -1.0, pb.Vr, Bp, sx, pb.hW + (long long)j * nc * mat, Bp, mat, 1.0, pb.Y, Bp, sx);
      if (j < n - 2) right_mult_Et(c, pb.Kst, Xn, pb.Y, 16, j, -1.0, +1, 1);  // Y -= chi_{j+1} E_j  (E_j[r][c] = K[(c, j), (r, j+1)])
      gemm(c, false, false, 16, Bp, Bp, 1.0, pb.Y, Bp, sx, pb.hS + (long long)j * nc * mat, Bp, mat, 0.0, Xc, Bp, sx);
      hipLaunchKernelGGL(k_store_corr, dim3(nblk(nc * (long long)G.t * G.b)), dim3(256), 0, st, G, Xc, corr, nc, j);
      std::swap(Xn, Xc);
    }
    launch_center_corr(c.ws, corr, nc, st);
  }
  // ---- K3
  hipLaunchKernelGGL(k_finalize, dim3(nblk(nc * G.t * G.t)), dim3(256), 0, st, G, pb.C0, pb.Gm, out, nc);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace hommx
