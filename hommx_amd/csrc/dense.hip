// dense.hip -- the batched dense kit both eliminations of the blocked family are made of (plane.hip, multifrontal.hip): fp64-MFMA GEMM
// tiles with their tile orders, and the recursive block inverse on 16 / 32 / 64 leaves that run in the registers of one wavefront.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "blocked_internal.h"
#include "sweep.h"

namespace hommx {

// ---------------------------------------------------------------------------------------------------------------
// batched fp64 MFMA GEMM  C = alpha op(A) op(B) + beta C  (v_mfma_f64_16x16x4_f64), TM x TM tile per
// workgroup of NW waves in a 2 x NW/2 grid: TM = 128, NW = 8 (64 x 32 per wave; 16 flop per byte of L2 -> LDS
// traffic) for M, N >= 256, TM = 64, NW = 4 for the small levels of the recursive inverse and the 16-row load
// products.  K is staged 16 at a time with the next stage prefetched into registers while the current one is
// multiplied; LDS pitch TM + 16 doubles (== 32 dwords mod 64: conflict-free ds_read_b64 fragments).  The grid is
// one-dimensional and XCD-aware: workgroup g runs on XCD g % 8 (round-robin dispatch), so
// cell = 8 * (slot / T) + g % 8 keeps ALL tiles of one cell on one XCD's 4 MB L2; symmetric updates enumerate the
// lower-triangle tiles only; an optional mirrored store (Ct) writes C^T as well, which replaces transpose passes.
// ---------------------------------------------------------------------------------------------------------------
template <bool TA, bool TB, int TM, int NW, bool GATHER = false>
__global__ __launch_bounds__(64 * NW, 2) void k_gemm_tile(int M, int N, int K, double alpha, const double* __restrict__ A,
                                                    int lda, long long sA, const double* __restrict__ B, int ldb,
                                                    long long sB, double beta, double* __restrict__ C, int ldc,
                                                    long long sC, int lowerOnly, int nc, int tilesX, int tilesPerCell,
                                                    double* Ct, GatherC ga = GatherC(), const int* __restrict__ tilemap = nullptr) {
  constexpr int PITCH = TM + 16;  // 2 PITCH dwords == 32 mod 64 for TM = 64 and 128: conflict-free ds_read_b64 fragments
  constexpr int WTM = TM / 2, WTN = TM / (NW / 2);  // per-wave tile: waves form a 2 x (NW / 2) grid
  constexpr int NFA = WTM / 16, NFB = WTN / 16;     // 16x16 MFMA tiles per wave, rows / columns
  constexpr int PT = TM * 16 / (64 * NW);           // doubles per thread, operand and 16-deep stage
  __shared__ double As[16 * PITCH];
  __shared__ double Bs[16 * PITCH];
  const int g = blockIdx.x, slot = g >> 3;
  const long long cell = 8ll * (slot / tilesPerCell) + (g & 7);
  if (cell >= nc) return;
  const int tile = slot % tilesPerCell;
  int ty, tx;
  if (tilemap) {  // lower triangle in super-blocks (gemm): the panels of a block stay in the XCD's L2
    ty = tilemap[tile] >> 16;
    tx = tilemap[tile] & 0xffff;
  } else if (lowerOnly) {  // tiles of the lower triangle, row by row
    ty = 0;
    while ((ty + 1) * (ty + 2) / 2 <= tile) ++ty;
    tx = tile - ty * (ty + 1) / 2;
  } else {
    ty = tile / tilesX;
    tx = tile % tilesX;
  }
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
  const int m0 = ty * TM, n0 = tx * TM;
  A += cell * sA;
  B += cell * sB;
  C += cell * sC;
  if (Ct) Ct += cell * sC;
  const int wi0 = WTM * (w / (NW / 2)), wj0 = WTN * (w % (NW / 2));
  const int l15 = l & 15, l4 = l >> 4;
  d4 acc[NFA][NFB];
#pragma unroll
  for (int a = 0; a < NFA; ++a)
#pragma unroll
    for (int b = 0; b < NFB; ++b) acc[a][b] = d4{0.0, 0.0, 0.0, 0.0};

  // staging maps.  "row-major along k" operand (A not transposed / B transposed): thread -> row t >> 1, 8 k's;
  // "k-major" operand (A transposed / B not transposed): thread -> k = t >> 4, 8 consecutive rows.
  constexpr int TPR = 16 / PT;   // threads per tile row in the row-major-along-k map
  constexpr int TPK = TM / PT;   // threads per k-row in the k-major map
  const int rk_row = tid / TPR, rk_k = (tid % TPR) * PT;
  const int km_k = tid / TPK, km_row = (tid % TPK) * PT;
  double pa[PT], pb[PT];
  auto fetch = [&](int k0) {
    const double* p;
    bool ok;
    if (!TA) { ok = m0 + rk_row < M; p = A + (long long)(m0 + rk_row) * lda + k0 + rk_k; }
    else     { ok = m0 + km_row < M; p = A + (long long)(k0 + km_k) * lda + m0 + km_row; }
#pragma unroll
    for (int x = 0; x < PT; x += 2) {
      double2 v = double2{0.0, 0.0};
      if (ok) v = *reinterpret_cast<const double2*>(p + x);
      pa[x] = v.x; pa[x + 1] = v.y;
    }
    if (TB) { ok = n0 + rk_row < N; p = B + (long long)(n0 + rk_row) * ldb + k0 + rk_k; }
    else    { ok = n0 + km_row < N; p = B + (long long)(k0 + km_k) * ldb + n0 + km_row; }
#pragma unroll
    for (int x = 0; x < PT; x += 2) {
      double2 v = double2{0.0, 0.0};
      if (ok) v = *reinterpret_cast<const double2*>(p + x);
      pb[x] = v.x; pb[x + 1] = v.y;
    }
  };
  auto stash = [&]() {
    if (!TA) {
#pragma unroll
      for (int x = 0; x < PT; ++x) As[(rk_k + x) * PITCH + rk_row] = pa[x];
    } else {
#pragma unroll
      for (int x = 0; x < PT; x += 2) *reinterpret_cast<double2*>(&As[km_k * PITCH + km_row + x]) = double2{pa[x], pa[x + 1]};
    }
    if (TB) {
#pragma unroll
      for (int x = 0; x < PT; ++x) Bs[(rk_k + x) * PITCH + rk_row] = pb[x];
    } else {
#pragma unroll
      for (int x = 0; x < PT; x += 2) *reinterpret_cast<double2*>(&Bs[km_k * PITCH + km_row + x]) = double2{pb[x], pb[x + 1]};
    }
  };

  fetch(0);
  stash();
  __syncthreads();
  // a diagonal tile of a GATHERING lower-triangle update (its epilogue stores nothing above the diagonal; the plain epilogue stores diagonal
  // tiles whole, and the recursive inverse reads them whole): the wave(s) whose sub-tile lies strictly above the diagonal -- wave 1 of the
  // 2 x 2 grid of a 64-tile -- keep staging operands and keeping the barriers, but issue no LDS reads and no MFMAs
  const bool idle = GATHER && lowerOnly && tx == ty && wj0 >= wi0 + WTM;
  for (int k0 = 0; k0 < K; k0 += 16) {
    const bool more = k0 + 16 < K;
    if (more) fetch(k0 + 16);
    if (!idle)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      double af[NFA], bf[NFB];
#pragma unroll
      for (int a = 0; a < NFA; ++a) af[a] = As[(4 * ks + l4) * PITCH + wi0 + 16 * a + l15];
#pragma unroll
      for (int b = 0; b < NFB; ++b) bf[b] = Bs[(4 * ks + l4) * PITCH + wj0 + 16 * b + l15];
#pragma unroll
      for (int a = 0; a < NFA; ++a)
#pragma unroll
        for (int b = 0; b < NFB; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[a], bf[b], acc[a][b], 0, 0, 0);
    }
    __syncthreads();
    if (more) {
      stash();
      __syncthreads();
    }
  }
  if constexpr (GATHER) {
    // multifrontal extend-add fused into the Schur update: C_out = sum over the child slots of U_child[map(row)][map(col)] + alpha acc
    // (valid entries of a child's update matrix are those on and below its diagonal: read through (max, min))
    const int f = (int)((cell + ga.batch0) % ga.nf);
    const long long mcell = (cell + ga.batch0) / ga.nf;
#pragma unroll
    for (int a = 0; a < NFA; ++a)
#pragma unroll
      for (int b = 0; b < NFB; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[a][b][r] *= alpha;
#pragma unroll 1
    for (int slot = 0; slot < 2; ++slot) {
      const MfChild ch = ga.child[f * 2 + slot];
      if (!ch.valid) continue;
      const int32_t* dp = ga.dpos + ((long long)f * 2 + slot) * ga.rp;
      const double* U = ga.arena + ga.nc * ch.offF + ((mcell * ch.nf + ch.fidx) * (long long)ch.L + ch.sp) * ch.L + ch.sp;
      int pc[NFB];
#pragma unroll
      for (int b = 0; b < NFB; ++b) {
        const int col = n0 + wj0 + 16 * b + l15;
        pc[b] = col < N ? dp[col] : -1;
      }
#pragma unroll
      for (int a = 0; a < NFA; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = m0 + wi0 + 16 * a + l4 + 4 * r;
          const int pr = row < M ? dp[row + ga.rowOff] : -1;
          if (pr < 0) continue;
#pragma unroll
          for (int b = 0; b < NFB; ++b)
            if (pc[b] >= 0 && !(lowerOnly && n0 + wj0 + 16 * b + l15 > row)) {
              const int hi = pr > pc[b] ? pr : pc[b], lo = pr > pc[b] ? pc[b] : pr;
              acc[a][b][r] += U[(long long)hi * ch.L + lo];
            }
        }
    }
#pragma unroll
    for (int a = 0; a < NFA; ++a)
#pragma unroll
      for (int b = 0; b < NFB; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = m0 + wi0 + 16 * a + l4 + 4 * r, col = n0 + wj0 + 16 * b + l15;
          if (row < M && col < N && !(lowerOnly && col > row)) C[(long long)row * ldc + col] = acc[a][b][r];  // above the diagonal: never read
        }
    return;
  }
#pragma unroll
  for (int a = 0; a < NFA; ++a)
#pragma unroll
    for (int b = 0; b < NFB; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wi0 + 16 * a + l4 + 4 * r, col = n0 + wj0 + 16 * b + l15;
        if (row < M && col < N) {
          double* p = C + (long long)row * ldc + col;
          double v = alpha * acc[a][b][r];
          if (beta != 0.0) v += beta * *p;
          *p = v;
          // mirrored copy (same leading dimension and batch stride as C).  With lowerOnly, Ct may be C itself: the tiles
          // below the diagonal then fill the ones above; diagonal tiles are complete and are not mirrored (two lanes
          // would write the same entry with values that differ in the last bit).
          if (Ct && !(lowerOnly && tx == ty)) Ct[(long long)col * ldc + row] = v;
        }
      }
}

// Super-block tile order of a lower triangle of `ty` tile rows (device table, cached per tile count).  The multifrontal route builds the
// tables of all its groups when its workspace is reserved (mf_reserve), so that no allocation or blocking copy happens while streams are
// being filled; a first use from anywhere else makes the table here.  A failed allocation falls back to the row-by-row order and leaves no
// sticky HIP error behind.
const int* ensure_tilemap(BlockedWorkspace* ws, int ty) {
  auto it = ws->tilemaps.find(ty);
  if (it != ws->tilemaps.end()) return it->second;
  const int SB = ws->tile_sb;
  std::vector<int> order;
  order.reserve((size_t)ty * (ty + 1) / 2);
  for (int I = 0; I < ty; I += SB)
    for (int J = 0; J <= I; J += SB)
      for (int i = I; i < std::min(I + SB, ty); ++i)
        for (int j = J; j < std::min(J + SB, ty) && j <= i; ++j) order.push_back(i << 16 | j);
  int* d = nullptr;
  if (hipMalloc(&d, sizeof(int) * order.size()) == hipSuccess &&
      hipMemcpy(d, order.data(), sizeof(int) * order.size(), hipMemcpyHostToDevice) == hipSuccess)
    return ws->tilemaps.emplace(ty, d).first->second;
  if (d) (void)hipFree(d);
  (void)hipGetLastError();  // the fallback is legitimate: do not let the failure surface later as somebody else's error
  return nullptr;
}

// tile size gemm() picks for an M x N (x K) product of this workspace: a gathering Schur update of rank below 1024 takes the 64 x 64 tiles
int gemm_tile_size(const BlockedWorkspace* ws, int M, int N, int K, bool gather) {
  return (M >= ws->gemm128_min && N >= ws->gemm128_min && !(gather && K < 1024)) ? 128 : 64;
}

void gemm(const Ctx& c, bool ta, bool tb, int M, int N, int K, double alpha, const double* A, int lda, long long sA,
          const double* B, int ldb, long long sB, double beta, double* C, int ldc, long long sC, int lowerOnly, double* Ct,
          const GatherC* gather) {
  // gemm128_min is a dev knob: smallest M, N routed to the 128x128 tiles (tests lower it to cover partial tiles); a gathering update of
  // small rank is bound by the traffic of the tiles it touches: 64-tiles waste less of the lower triangle
  const int TM = gemm_tile_size(c.ws, M, N, K, gather != nullptr);
  const bool big = TM == 128;
  const int tx = (N + TM - 1) / TM, ty = (M + TM - 1) / TM;
  const int T = lowerOnly ? ty * (ty + 1) / 2 : tx * ty;
  const long long groups = (c.nc + 7) / 8;
  {  // a launch holds at most 2^32 - 1 work-items (AQL grid size): huge batches go in pieces
    const long long max_groups = std::max(1ll, (1ll << 30) / (8ll * T * (big ? 512 : 256)));
    if (groups > max_groups) {
      for (long long g0 = 0; g0 < groups; g0 += max_groups) {
        Ctx sub = c;
        const long long b0 = g0 * 8;
        sub.nc = std::min(c.nc - b0, max_groups * 8);
        GatherC gs;
        if (gather) {
          gs = *gather;
          gs.batch0 = gather->batch0 + b0;
        }
        gemm(sub, ta, tb, M, N, K, alpha, A + b0 * sA, lda, sA, B + b0 * sB, ldb, sB, beta, C + b0 * sC, ldc, sC, lowerOnly,
             Ct ? Ct + b0 * sC : nullptr, gather ? &gs : nullptr);
      }
      return;
    }
  }
  // Big lower-triangle updates walk their tiles in SB x SB super-blocks: row by row a tile row of a 1,536-front touches 8 MB of B panels,
  // twice an XCD's L2, and every panel is fetched once per tile (the rank-672 update of C4 fetched 143 MB per cell for 52 MB of operands)
  const int* tilemap = (lowerOnly && c.ws->tile_sb > 1 && ty >= 2 * c.ws->tile_sb) ? ensure_tilemap(c.ws, ty) : nullptr;
  dim3 grid((unsigned)(groups * 8 * T));
  // 128 tiles: 8 waves per workgroup (2 x 4 grid of 64 x 32 wave tiles, 110 VGPRs, 4 waves per SIMD): +2 % over 4 waves
  // of 64 x 64; 64 tiles: 4 waves of 32 x 32 (8 waves measured slower)
  auto launch = [&](auto TA, auto TB, auto GA) {  // a gathering update (virtual C, multifrontal.hip) is NN only
    const GatherC ga = GA() ? *gather : GatherC();
    if (big)
      hipLaunchKernelGGL((k_gemm_tile<TA(), TB(), 128, 8, GA()>), grid, dim3(512), 0, c.st, M, N, K, alpha, A, lda, sA, B, ldb, sB, beta, C,
                         ldc, sC, lowerOnly, (int)c.nc, tx, T, Ct, ga, tilemap);
    else
      hipLaunchKernelGGL((k_gemm_tile<TA(), TB(), 64, 4, GA()>), grid, dim3(256), 0, c.st, M, N, K, alpha, A, lda, sA, B, ldb, sB, beta, C,
                         ldc, sC, lowerOnly, (int)c.nc, tx, T, Ct, ga, tilemap);
  };
  const std::false_type no;
  const std::true_type yes;
  if (gather) launch(no, no, yes);
  else if (!ta && !tb) launch(no, no, no);
  else if (!ta && tb) launch(no, yes, no);
  else if (ta && !tb) launch(yes, no, no);
  else launch(yes, yes, no);
}

// OUT[i][j] = IN[j][i]  (sub-blocks, batched)
__global__ void k_transpose(int M, int N, const double* __restrict__ IN, int ldi, long long sI, double* __restrict__ OUT,
                            int ldo, long long sO, long long ncells) {
  const long long per = (long long)M * N;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= ncells * per) return;
  const long long cell = idx / per;
  const int rem = (int)(idx % per);
  const int j = rem % N, i = rem / N;
  OUT[cell * sO + (long long)i * ldo + j] = IN[cell * sI + (long long)j * ldi + i];
}

// in-place inverse of the NB x NB SPD diagonal sub-block at (off, off): one wavefront per cell
template <int NB>
__global__ __launch_bounds__(64) void k_leaf_inverse(double* __restrict__ S, int ld, long long stride, int off,
                                                     int32_t* __restrict__ info, int stepcode, int infoDiv) {
  constexpr int RPL = Cfg<NB>::RPL;
  __shared__ alignas(16) double ubuf[NB];
  __shared__ alignas(16) double wbuf[NB];
  const long long cell = blockIdx.x;
  const int l = threadIdx.x, c = l % NB, g = l / NB, r0 = g * RPL;
  double* P = S + cell * stride + (long long)off * ld + off;
  double s[RPL];
#pragma unroll
  for (int i = 0; i < RPL; ++i) s[i] = P[(long long)(r0 + i) * ld + c];
  int bad = 0;
  SweepStep<NB, 0>::run(s, ubuf, wbuf, c, g, r0, bad);
#pragma unroll
  for (int i = 0; i < RPL; ++i) P[(long long)(r0 + i) * ld + c] = -s[i];
  if (bad && l == 0 && info) atomicCAS(&info[cell / infoDiv], 0, stepcode);
}

// same for NB = 64 in the block layout of sweep_blk (lane = 8x8 block, 128 VGPRs of matrix): one launch instead of the
// two 32-leaves, four GEMMs and their launch latencies of a 64-node of the recursion.  Reads the LOWER triangle only
// (blocks above the diagonal are mirrored on the way in), writes the full symmetric inverse.
template <int NB>
__global__ __launch_bounds__(64) void k_leaf_inverse_blk(double* __restrict__ S, int ld, long long stride, int off,
                                                         int32_t* __restrict__ info, int stepcode, int infoDiv) {
  constexpr int BS = NB / 8;
  __shared__ alignas(16) double ubuf[NB];
  const long long cell = blockIdx.x;
  const int l = threadIdx.x, bi = l >> 3, bj = l & 7;
  double* P = S + cell * stride + (long long)off * ld + off;
  double s[BS * BS];
#pragma unroll
  for (int r = 0; r < BS; ++r)
#pragma unroll
    for (int q = 0; q < BS; ++q) {
      const int row = BS * bi + r, col = BS * bj + q;
      s[r * BS + q] = (bi >= bj) ? P[(long long)row * ld + col] : P[(long long)col * ld + row];
    }
  int bad = 0;
  sweep_blk<NB>(s, ubuf, bi, bj, bad);
#pragma unroll
  for (int r = 0; r < BS; ++r)
#pragma unroll
    for (int q = 0; q < BS; ++q) P[(long long)(BS * bi + r) * ld + BS * bj + q] = -s[r * BS + q];
  if (bad && l == 0 && info) atomicCAS(&info[cell / infoDiv], 0, stepcode);
}

// in-place inverse of the SPD diagonal block [off, off+size) of every matrix of the batch (ld / batch stride from the context,
// default Bp / Bp^2), recursive Schur-complement form; `tmp` points at free scratch (consumed stack-like by the nesting levels)
void invert(const Ctx& c, double* S, int off, int size, double* tmp) {
  const Geo& G = c.ws->G;
  const int ld = c.ld ? c.ld : G.Bp;
  const long long sS = c.sS ? c.sS : (long long)G.Bp * G.Bp;
  const long long sT = c.sT ? c.sT : sS;
  if (size <= 32) {
    if (size == 32)
      hipLaunchKernelGGL(k_leaf_inverse<32>, dim3((unsigned)c.nc), dim3(64), 0, c.st, S, ld, sS, off, c.info, c.stepcode, c.infoDiv);
    else
      hipLaunchKernelGGL(k_leaf_inverse<16>, dim3((unsigned)c.nc), dim3(64), 0, c.st, S, ld, sS, off, c.info, c.stepcode, c.infoDiv);
    return;
  }
  if (size == 64) {
    hipLaunchKernelGGL(k_leaf_inverse_blk<64>, dim3((unsigned)c.nc), dim3(64), 0, c.st, S, ld, sS, off, c.info, c.stepcode, c.infoDiv);
    return;
  }
  int s1 = (size / 2) / 32 * 32;
  if (s1 < 32) s1 = 32;
  if (size >= 128 && size % 64 == 0) s1 = (size / 2) / 64 * 64;  // 192 -> 64 + 128: every leaf a 64-block, whole 64-tiles
  const int s2 = size - s1;
  double* A11 = S + (long long)off * ld + off;
  double* A21 = S + (long long)(off + s1) * ld + off;
  double* A12 = S + (long long)off * ld + off + s1;
  double* A22 = S + (long long)(off + s1) * ld + off + s1;
  double* Xm = tmp;  // s2 x s1, ld = s1, batch stride sT
  invert(c, S, off, s1, tmp);                                                  // A11 <- A11^-1
  gemm(c, false, false, s2, s1, s1, 1.0, A21, ld, sS, A11, ld, sS, 0.0, Xm, s1, sT);   // Xm = A21 A11^-1
  gemm(c, false, true, s2, s2, s1, -1.0, Xm, s1, sT, A21, ld, sS, 1.0, A22, ld, sS, 1);  // A22 <- A22 - Xm A21^T (symmetric: lower tiles;
                                                                                          //  the recursion below never reads above the diagonal tiles)
  invert(c, S, off + s1, s2, tmp + (long long)s1 * s2);                        // A22 <- (Schur)^-1
  gemm(c, false, false, s2, s1, s2, -1.0, A22, ld, sS, Xm, s1, sT, 0.0, A21, ld, sS, 0, A12);  // A21 <- -T^-1 Xm, A12 <- A21^T
  gemm(c, true, false, s1, s1, s2, -1.0, Xm, s1, sT, A21, ld, sS, 1.0, A11, ld, sS, 1, A11);  // A11 <- A11^-1 - Xm^T A21: symmetric
                                                                         // (= A11^-1 + Xm^T T^-1 Xm): lower tiles, mirrored in place
}

}  // namespace hommx
